"""Time from a computed sharded table to a served path cache on C4, two ways,
for K logical row shards on one device (K in --shards, default 1 2 8):

  (a) another build of the library (--base-lib, e.g.
      shadow-1_amd/libshdpe_head.so from tools/build_head.sh, loaded through
      SHDPE_LIB): Engine.gather() then Engine.fill_rowstore;
  (b) the in-tree library: Engine.fill_rowstore_shards, no gather.

Every measurement is a child process (one library per process).  A sample is
a fresh engine with K shards, compute_all, then the timed call(s) into an
empty store; the first sample of a child is a warm-up.  (a) and (b) children
alternate, --rounds of each per K; a round's figure is the median of its
samples.  Reported per K and leg: median / min / max over the rounds of the
wall total and its parts, (b)'s info fields, and "b_within_a_spread": (b)'s
median total is no larger than (a)'s median plus (a)'s own min-to-max spread.

  python tools/fill_shards_time.py --base-lib shadow-1_amd/libshdpe_head.so \
      [--rounds 5] [--samples 2] [--flags 0] [--out profiles/fill_shards_c4.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "shadow-1_amd"))


def child(workload, K, samples, flags, leg):
    from shdpe import generators as G
    from shdpe.engine import Engine, RowStore
    top, att = G.make_config(workload)
    out = []
    for i in range(samples + 1):
        eng = Engine(top, att, devices=[0] * K)
        eng.compute_all()
        st = RowStore(top.n, eng.attached)
        t0 = time.perf_counter()
        if leg == "a":
            if K > 1:
                eng.gather()
            t1 = time.perf_counter()
            _, ms = eng.fill_rowstore(st, fill_flags=flags)
            rec = {"gather": (t1 - t0) * 1e3, "fill": (time.perf_counter() - t1) * 1e3,
                   "compute": ms["alloc"], "pack": ms["pack"], "dma": ms["dma"]}
        else:
            _, info = eng.fill_rowstore_shards(st, fill_flags=flags)
            rec = {"compute": info["msCompute"], "pack": info["msPack"], "dma": info["msDma"],
                   "resolve": info["msResolve"],
                   "info": {k: info[k] for k in ("shards", "fromFullTable", "needs", "needsStored", "needRounds",
                                                 "deviceBytesPeak")}}
        rec["total"] = (time.perf_counter() - t0) * 1e3
        rec["entries"] = int(st.size())
        st.close()
        eng.close()
        if i:
            out.append(rec)
    print("RESULT " + json.dumps(out), flush=True)


def run_child(args, lib, K, leg):
    env = dict(os.environ)
    env.pop("SHDPE_LIB", None)
    if lib:
        env["SHDPE_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", leg, "--workload", args.workload,
           "--samples", str(args.samples), "--flags", str(args.flags), "--shards", str(K)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.child_timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"child failed with status {r.returncode}: stopping")
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def summary(rounds, keys):
    return {k: {"median": statistics.median(x[k] for x in rounds), "min": min(x[k] for x in rounds),
                "max": max(x[k] for x in rounds)} for k in keys}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--base-lib", help="library build for leg (a)")
    ap.add_argument("--workload", default="c4")
    ap.add_argument("--shards", type=int, nargs="+", default=[1, 2, 8])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--samples", type=int, default=2)
    ap.add_argument("--flags", type=int, default=0, help="fill flag word (1 prefer direct, 2 direct pairs)")
    ap.add_argument("--child-timeout", type=float, default=300.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fill_shards_c4.json"))
    ap.add_argument("--child", choices=["a", "b"], help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.workload, args.shards[0], args.samples, args.flags, args.child)
    if not args.base_lib or not os.path.exists(args.base_lib):
        raise SystemExit("--base-lib: the library build to compare against (tools/build_head.sh)")
    KA, KB = ("gather", "fill", "pack", "dma", "total"), ("pack", "dma", "resolve", "total")
    out = {"workload": args.workload, "rounds": args.rounds, "samples_per_round": args.samples,
           "fill_flags": args.flags,
           "unit": "ms wall; per round the median of its samples, then median / min / max over rounds",
           "note": "logical shards on one device: the distinct-device path (concurrent PCIe transfers) is unmeasured",
           "shards": {}}
    for K in args.shards:
        a, b, info, entries = [], [], None, None
        for r in range(args.rounds):
            ra = run_child(args, args.base_lib, K, "a")
            rb = run_child(args, None, K, "b")
            a.append({k: statistics.median(x[k] for x in ra) for k in KA})
            b.append({k: statistics.median(x[k] for x in rb) for k in KB})
            info, entries = rb[0]["info"], (ra[0]["entries"], rb[0]["entries"])
            print(f"K={K} round {r}: total ms  a {a[-1]['total']:.1f} (gather {a[-1]['gather']:.1f})  "
                  f"b {b[-1]['total']:.1f}", flush=True)
        sa, sb = summary(a, KA), summary(b, KB)
        spread = sa["total"]["max"] - sa["total"]["min"]
        out["shards"][str(K)] = {
            "a_base_gather_plus_fill": sa, "b_fill_rowstore_shards": sb, "b_info": info,
            "entries_a_b": entries,
            "b_within_a_spread": sb["total"]["median"] <= sa["total"]["median"] + spread,
            "per_round": {"a": a, "b": b}}
        # written after every K: a run cut short keeps what it measured
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({K: {"a": v["a_base_gather_plus_fill"]["total"], "b": v["b_fill_rowstore_shards"]["total"],
                          "b_within_a_spread": v["b_within_a_spread"]} for K, v in out["shards"].items()}))


if __name__ == "__main__":
    main()
