"""Wall time of creating the engine, three ways, on one box:

  (a) shd_pe_create of another build of the library (--base-lib, e.g.
      shadow-1_amd/libshdpe_head.so from tools/build_head.sh: the parent
      commit), loaded through SHDPE_LIB;
  (b) the tree's host build  (shd_pe_create_built, SHD_PE_BUILD_HOST);
  (c) the tree's device build (SHD_PE_BUILD_DEVICE), with ShdPeBuildInfo's
      splits.

Every measurement is a child process (one library per process): the graph is
generated, one cold construction, then --warm timed constructions (create +
destroy).  The tree's child alternates (c) and (b).  (a) and tree children
alternate, --rounds of each.  Shapes: the C3a, C3b and C4 configurations and
complete graphs with a loop on every vertex (kN: n = N).

SHD_PE_BUILD_AUTO's threshold is derived here: the smallest measured edge count
of a complete graph from which on the device build's median beats the host
build's by more than the run-to-run spread (the larger of the two max - min
ranges at that shape), at that shape and at every larger one.  null: no such
shape, auto stays on the host build.

  python tools/create_time.py --base-lib shadow-1_amd/libshdpe_head.so \
      [--shapes c3a,c3b,c4,k1000,k2500,k5000,k10000] [--rounds 2] [--warm 3] \
      [--out profiles/create_device_build.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "shadow-1_amd"))

SHAPES = "c3a,c3b,c4,k1000,k2500,k5000,k10000"


def make_shape(name):
    import numpy as np
    from shdpe import generators as G
    if name.startswith("k"):
        top = G.dense(int(name[1:]), seed=3)
        return top, np.arange(top.n, dtype=np.int32)
    return G.make_config(name)


def child(shape, warm, tree):
    from shdpe import engine as E
    t0 = time.perf_counter()
    top, att = make_shape(shape)
    gen_s = time.perf_counter() - t0

    def one(build):
        t0 = time.perf_counter()
        eng = E.Engine(top, att, graph_build=build)
        ms = (time.perf_counter() - t0) * 1e3
        st = eng.stats()
        info = eng.build_info() if build is not None else {}
        eng.close()
        return dict(info, wall=ms, nArcs=int(st["nArcs"]), mode=int(st["mode"]))

    out = {"shape": shape, "n": int(top.n), "edges": int(top.m), "gen_s": gen_s}
    if tree:
        out["cold_host"] = one(E.BUILD_HOST)
        out["cold_device"] = one(E.BUILD_DEVICE)
        out["device"], out["host"] = [], []
        for _ in range(warm):
            out["device"].append(one(E.BUILD_DEVICE))
            out["host"].append(one(E.BUILD_HOST))
    else:
        out["cold_base"] = one(None)
        out["base"] = [one(None) for _ in range(warm)]
    print("RESULT " + json.dumps(out), flush=True)


def run_child(args, shape, lib):
    env = dict(os.environ)
    env.pop("SHDPE_LIB", None)
    if lib:
        env["SHDPE_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--shapes", shape, "--warm", str(args.warm)]
    if not lib:
        cmd.append("--tree")
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.child_timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"child failed with status {r.returncode}: stopping")
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def summary(runs, key="wall"):
    xs = [x[key] for x in runs]
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": len(xs)}


def auto_threshold(shapes):
    """See the module text; the complete graphs only (the shape the device build is for)."""
    comp = sorted((s for s in shapes.values() if s["complete"]), key=lambda s: s["edges"])
    wins = []
    for s in comp:
        spread = max(s["host_ms"]["max"] - s["host_ms"]["min"], s["device_ms"]["max"] - s["device_ms"]["min"])
        wins.append({"shape": s["shape"], "edges": s["edges"], "host_median": s["host_ms"]["median"],
                     "device_median": s["device_ms"]["median"], "spread": spread,
                     "device_wins": s["device_ms"]["median"] < s["host_ms"]["median"] - spread})
    thr = None
    for k in range(len(wins) - 1, -1, -1):
        if not wins[k]["device_wins"]:
            break
        thr = wins[k]["edges"]
    return thr, wins


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--base-lib", help="library build for variant (a)")
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--big-rounds", type=int, default=1, help="rounds at the C3 shapes (a minute per child)")
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--child-timeout", type=float, default=600.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "create_device_build.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.shapes, args.warm, args.tree)
    if not args.base_lib or not os.path.exists(args.base_lib):
        raise SystemExit("--base-lib: the library build to compare against (tools/build_head.sh)")
    shapes = {}
    for shape in args.shapes.split(","):
        base, host, dev, cold = [], [], [], {}
        rounds = args.big_rounds if shape.startswith("c3") else args.rounds
        for r in range(rounds):
            ra = run_child(args, shape, args.base_lib)
            rt = run_child(args, shape, None)
            base += ra["base"]
            host += rt["host"]
            dev += rt["device"]
            cold = {"base": ra["cold_base"]["wall"], "host": rt["cold_host"]["wall"],
                    "device": rt["cold_device"]["wall"]}
            print(f"{shape} round {r}: base {summary(ra['base'])['median']:.1f}  host "
                  f"{summary(rt['host'])['median']:.1f}  device {summary(rt['device'])['median']:.1f} ms "
                  f"(graph generated in {rt['gen_s']:.1f} s)", flush=True)
        d0 = dev[0]
        shapes[shape] = {
            "shape": shape, "n": rt["n"], "edges": rt["edges"], "nArcs": d0["nArcs"], "mode": d0["mode"],
            "complete": shape == "c3a" or shape.startswith("k"),
            "base_ms": summary(base), "host_ms": summary(host), "device_ms": summary(dev), "cold_ms": cold,
            "device_built": d0["built"], "device_handedOff": d0["handedOff"], "device_handOffWhy": d0["handOffWhy"],
            "device_bytes_peak": d0["deviceBytesPeak"],
            "device_splits_ms": {k: summary(dev, k) for k in ("msUpload", "msKernels", "msReadback", "msCreate")},
            "host_splits_ms": {k: summary(host, k) for k in ("msHostBuild", "msCreate")},
            "host_within_base_spread": summary(base)["min"] <= summary(host)["median"] <= summary(base)["max"],
        }
    thr, wins = auto_threshold(shapes)
    out = {"unit": "wall ms of create + destroy in a warm process; median / min / max over all warm runs of "
                   "all rounds; cold_ms: the first construction of the last round's processes",
           "rounds": args.rounds, "big_rounds": args.big_rounds, "warm_per_round": args.warm,
           "auto_threshold_edges": thr,
           "auto_threshold_derivation": {
               "rule": "smallest complete-graph edge count from which on device median < host median - spread, "
                       "spread = the larger max - min range of the two at that shape",
               "shapes": wins},
           "shapes": shapes}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({"auto_threshold_edges": thr, "wins": wins}))


if __name__ == "__main__":
    main()
