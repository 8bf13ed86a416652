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

--parent-tier switches the parent tier on (shd_pe_table_load_set_parent_tier)
in legs a, d and counters, for the engines the tree tier does not cover (C2:
the per-row sparse kernel) or covers in part (c4q: the tie rows with a slot).
Leg b stays the request route alone, and one leg joins the protocol: d_off, leg
d with the tier off.

--config c3b (the dense mode: 20,000 vertices one edge short of complete, all
attached; SHDPE_C3_N overrides n, and the n used is written into the file) runs
its own protocol with the parent tier on, into profiles/dense_tier_c3bshape.json:

  a         rows [0, 256) with a seeded random weight matrix, parent tier on
  b_trial   16 of those rows with the tier off, one timed call: leg b's limit is
            sized from it, linearly in the sources
  b         leg a's rows with the tier off: every source by the request route.
            Where the trial says that takes more than 20 minutes, legs b and
            a_16 run on 16 rows instead and the file says so
  d         all rows with weight == NULL, beside compute_all of the same process
  d_q       the same on c3bq (quantized latencies: tie rows over the dense slots)

(a), (b) and (c) must give identical sums (sha256 over arc, vertex and totals,
kept in the file); (a) is expected below (b) and (c) by more than the sum of
their min-max spreads, and the file says whether it is (`*_by_more_than_spreads`,
`*_ratio_device`: the slower leg's median over the faster's).  --legs runs a
part of the protocol; every check applies to the legs that ran.

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
    if args.parent_tier:
        eng.set_table_load_parent_tier(True)
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
           "info": {k: info[k] for k in ("tree", "direct", "route", "handed_on", "claimed", "rounds", "atomics",
                                         "parents", "tie", "parent_claimed", "parent_atomics")},
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
    res = _result(eng, out, wall, dev, {"sources": rows, "requests": rows * eng.T, "vertices": eng.top.n})
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
    res = _result(eng, out, wall, dev, {"sources": eng.T, "requests": eng.T * eng.T, "compute_all_ms": st["msTotal"],
                                        "vertices": eng.top.n, "rows_exact": st["rowsExact"]})
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
    "d_off": lambda args: {"d_parent_tier_off": step_d(args)},
    "once": step_once,
}


DENSE_CONFIGS = ("c3b", "c3bq")
DENSE_SOURCES, DENSE_TRIAL, DENSE_B_LIMIT = 256, 16, 1200


def _child(args, step, env, key=None, **over):
    """One step as a child under its own `timeout` -> its result, under `key`
    where given.  over: the child's config / sources / repeats / timeout /
    parent_tier where they differ from the protocol's."""
    a = {**vars(args), **over}
    part = f"{args.out}.{step}.part"
    cmd = ["timeout", "-k", "10", str(a["step_timeout"]), sys.executable, os.path.abspath(__file__),
           "--config", a["config"], "--step", step, "--out", part, "--repeats", str(a["repeats"]),
           "--sources", str(a["sources"]), "--block", str(a["block"])]
    if a["parent_tier"]:
        cmd.append("--parent-tier")
    t0 = time.perf_counter()
    rc = subprocess.run(cmd, env={**os.environ, **env}).returncode
    if rc:
        raise SystemExit(f"step {step}: exit status {rc}; no further step was started")
    with open(part) as f:
        res = json.load(f)
    os.remove(part)
    if key:
        (leg,) = res.values()
        leg["child_wall_s"] = time.perf_counter() - t0
        res = {key: leg}
    return res


def run_dense(args):
    """The dense protocol (the docstring's --config c3b part)."""
    legs = args.legs.split(",") if args.legs else ["a", "b", "d", "d_q"]
    res = {"config": args.config, "unit": "ms", "parent_tier": True}
    rows = min(args.sources, DENSE_SOURCES)
    if "a" in legs:
        res.update(_child(args, "a", {}, sources=rows, parent_tier=True))
    if "b" in legs:
        res.update(_child(args, "b", {}, key="b_trial", sources=DENSE_TRIAL, repeats=1, parent_tier=False))
        t = res["b_trial"]
        per_call_s = t["wall_ms"]["median"] / 1e3 * rows / t["sources"]
        setup_s = max(0.0, t["child_wall_s"] - 2 * t["wall_ms"]["median"] / 1e3)
        need_s = setup_s + (1 + args.repeats) * per_call_s
        res["b_extrapolated_s"] = need_s
        if need_s > DENSE_B_LIMIT:
            rows_b = DENSE_TRIAL
            res["b_note"] = (f"the request route on {rows} sources extrapolates to {need_s:.0f} s, past "
                             f"{DENSE_B_LIMIT} s: legs b and a_16 ran on {rows_b} sources, and a_below_b compares those")
            res.update(_child(args, "a", {}, key="a_16", sources=rows_b, parent_tier=True))
            need_s = setup_s + (1 + args.repeats) * t["wall_ms"]["median"] / 1e3
        else:
            rows_b = rows
        limit = int(min(DENSE_B_LIMIT, 60 + 1.5 * need_s))
        res["b_timeout_s"] = limit
        res.update(_child(args, "b", {}, sources=rows_b, parent_tier=False, step_timeout=limit))
    if "d" in legs:
        res.update(_child(args, "d", {}, parent_tier=True))
    if "d_q" in legs:
        res.update(_child(args, "d", {}, key="d_q_all_rows_unit_weight", config="c3bq", parent_tier=True))
    used = {leg["vertices"] for leg in res.values() if isinstance(leg, dict) and "vertices" in leg}
    res["vertices"] = sorted(used)[0] if len(used) == 1 else sorted(used)
    return res


def run_steps(args):
    if args.config in DENSE_CONFIGS:
        return finish(args, run_dense(args))
    plan = [("a", {}), ("b", {"SHDPE_TLOAD_TREE": "0"}), ("c", {}), ("d", {})]
    if args.leg_e:
        plan.append(("e", {}))
    if args.counters:
        plan.append(("counters", {}))
    if args.parent_tier:
        plan.append(("d_off", {}))
    if args.legs:
        plan = [(step, env) for step, env in plan if step in args.legs.split(",")]
    res = {"config": args.config, "unit": "ms", "parent_tier": bool(args.parent_tier)}
    for step, env in plan:
        res.update(_child(args, step, env, parent_tier=args.parent_tier and step not in ("b", "c", "d_off")))
    finish(args, res)


def finish(args, res):
    """The checks over the legs that ran, and the file."""
    spread = lambda r: r["device_ms"]["max"] - r["device_ms"]["min"]
    fast = lambda r: r["info"]["tree"] + r["info"]["parents"] + r["info"]["tie"]

    def same_sums(keys):
        """The legs of `keys` that ran gave identical sums."""
        digests = {k: res[k]["digest"] for k in keys if k in res}
        if len(set(digests.values())) > 1:
            raise SystemExit(f"legs give different sums: {digests}")
        return sorted(digests)

    def below(fast_leg, slow_leg, name):
        """fast_leg's median device time below slow_leg's by more than both min-max spreads."""
        if fast_leg not in res or slow_leg not in res:
            return
        f, o = res[fast_leg], res[slow_leg]
        res[f"{name}_by_more_than_spreads"] = bool(
            o["device_ms"]["median"] - f["device_ms"]["median"] > spread(f) + spread(o))
        res[f"{name}_ratio_device"] = o["device_ms"]["median"] / f["device_ms"]["median"]

    a_leg = "a_16" if "a_16" in res else "a_tree"     # (the dense protocol's leg b on fewer sources)
    res["sums_equal_first_rows"] = same_sums((a_leg, "b_route", "c_path_load"))
    res["sums_equal_all_rows"] = same_sums(("d_all_rows_unit_weight", "d_parent_tier_off"))
    if "a_tree" in res and fast(res["a_tree"]) == 0:
        raise SystemExit(f"no fast tier served leg a: {res['a_tree']['info']}")
    if "b_route" in res and fast(res["b_route"]) != 0:
        raise SystemExit(f"the tier switches did not take in leg b: {res['b_route']['info']}")
    below(a_leg, "b_route", "a_below_b")
    below("a_tree", "c_path_load", "a_below_c")
    below("d_all_rows_unit_weight", "d_parent_tier_off", "d_below_d_off")
    if "a_counters" in res:
        i = res["a_counters"]["info"]
        res["commit_global_adds_per_claimed_entry"] = (i["atomics"] + i["parent_atomics"]) / max(
            1, i["claimed"] + i["parent_claimed"])
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
    ap.add_argument("--parent-tier", action="store_true",
                    help="switch the parent tier on in legs a, d and counters; adds leg d_off")
    ap.add_argument("--legs", default=None, help="run only these steps of the protocol (comma-separated)")
    ap.add_argument("--out", default=None, help="default: profiles/table_load_<config>shape.json")
    args = ap.parse_args()
    if args.out is None:
        name = "dense_tier_c3bshape.json" if args.config in DENSE_CONFIGS else f"table_load_{args.config}shape.json"
        args.out = os.path.join(ROOT, "profiles", name)
    if args.step:
        res = STEPS[args.step](args)
        with open(args.out, "w") as f:
            json.dump(res, f)
        return
    run_steps(args)


if __name__ == "__main__":
    main()
