"""Pack / DMA time of the one-call path-cache fill on C4, three variants:

  (a) shd_pe_fill_rowstore of another build of the library (--base-lib, e.g.
      shadow-1_amd/libshdpe_head.so from tools/build_head.sh), loaded through
      SHDPE_LIB;
  (b) the same call of the in-tree library;
  (c) shd_pe_fill_rowstore_ex with PREFER_DIRECT | DIRECT_PAIRS, in-tree.

Every measurement is a child process (one library per process): engine on
C4, compute_all, one warm-up fill, then --fills timed fills into fresh
stores.  (a) and (b) children alternate, --rounds of each; (c) is timed in
(b)'s child after its plain fills, so (a) and (b) run the same sequence.  The zero-flag path is meant
to be the same code, so (b)'s median pack time must lie within the spread
(a)'s rounds show against each other in this same run: "b_within_a_spread".

  python tools/fill_direct_bench.py --base-lib shadow-1_amd/libshdpe_head.so \
      [--rounds 5] [--fills 3] [--out profiles/fill_direct_c4.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "shadow-1_amd"))


def child(workload, fills, with_ex):
    from shdpe import generators as G
    from shdpe.engine import Engine, RowStore
    top, att = G.make_config(workload)
    eng = Engine(top, att)
    eng.compute_all()

    def one(**kw):
        st = RowStore(top.n, eng.attached)
        t0 = time.perf_counter()
        _, ms = eng.fill_rowstore(st, **kw)
        ms = dict(ms, total=(time.perf_counter() - t0) * 1e3, entries=int(st.size()),
                  image_bytes=int(st.memory_bytes()))
        st.close()
        return ms

    # (a) and (b) must see the same sequence: the plain fills back to back
    # first, the flagged ones only after them
    one()                                               # warm-up
    out = {"plain": [one() for _ in range(fills)], "ex": []}
    if with_ex:
        one(prefers_direct=True, direct_pairs=True)     # warm-up (uploads posOf)
        out["ex"] = [one(prefers_direct=True, direct_pairs=True) for _ in range(fills)]
    eng.close()
    print("RESULT " + json.dumps(out), flush=True)


def run_child(args, lib, with_ex):
    env = dict(os.environ)
    env.pop("SHDPE_LIB", None)
    if lib:
        env["SHDPE_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--workload", args.workload,
           "--fills", str(args.fills)] + (["--with-ex"] if with_ex else [])
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.child_timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"child failed with status {r.returncode}: stopping")
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def med(runs, key):
    return statistics.median(x[key] for x in runs)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--base-lib", help="library build for variant (a)")
    ap.add_argument("--workload", default="c4")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--fills", type=int, default=3)
    ap.add_argument("--child-timeout", type=float, default=240.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fill_direct_c4.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--with-ex", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.workload, args.fills, args.with_ex)
    if not args.base_lib or not os.path.exists(args.base_lib):
        raise SystemExit("--base-lib: the library build to compare against (tools/build_head.sh)")
    a, b, c = [], [], []
    for r in range(args.rounds):
        ra = run_child(args, args.base_lib, False)
        rb = run_child(args, None, True)
        a.append({k: med(ra["plain"], k) for k in ("pack", "dma", "total")})
        b.append({k: med(rb["plain"], k) for k in ("pack", "dma", "total")})
        c.append({k: med(rb["ex"], k) for k in ("pack", "dma", "total")})
        shape = {"entries_plain": rb["plain"][0]["entries"], "entries_ex": rb["ex"][0]["entries"],
                 "image_bytes_plain": rb["plain"][0]["image_bytes"],
                 "image_bytes_ex": rb["ex"][0]["image_bytes"]}
        print(f"round {r}: pack ms  a {a[-1]['pack']:.2f}  b {b[-1]['pack']:.2f}  c {c[-1]['pack']:.2f}",
              flush=True)

    def summary(rounds):
        return {k: {"median": statistics.median(x[k] for x in rounds), "min": min(x[k] for x in rounds),
                    "max": max(x[k] for x in rounds)} for k in ("pack", "dma", "total")}

    sa, sb, sc = summary(a), summary(b), summary(c)
    out = {"workload": args.workload, "rounds": args.rounds, "fills_per_round": args.fills,
           "unit": "ms; per round the median of its fills, then median / min / max over rounds",
           "a_base_fill_rowstore": sa, "b_head_fill_rowstore": sb, "c_head_fill_ex_prefer_direct_pairs": sc,
           "b_within_a_spread": sa["pack"]["min"] <= sb["pack"]["median"] <= sa["pack"]["max"],
           "c_pack_over_b_pack": sc["pack"]["median"] / sb["pack"]["median"], **shape,
           "per_round": {"a": a, "b": b, "c": c}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in ("a_base_fill_rowstore", "b_head_fill_rowstore",
                                          "c_head_fill_ex_prefer_direct_pairs", "b_within_a_spread",
                                          "c_pack_over_b_pack")}))


if __name__ == "__main__":
    main()
