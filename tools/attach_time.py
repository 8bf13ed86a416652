"""Time of host attachment at the north-star shape: V = 100,000 vertices,
16,384 hosts, generator attributes and hints (shdpe.generators.vertex_attrs /
attach_hints).  One process, two measurements:

  batched   Attacher.attach (shd_pe_attach_hosts): after a warm-up call, enough
            repetitions to fill about a second; per call the device time of its
            kernels (events around them) and the wall time of the whole call,
            staging included.
  host      shd_pe_attach_host, the one-query loop, over a 256-host sample on
            one thread, scaled to 16,384 hosts.

The comparison point is the host one-query loop on the same box: Shadow's own
topology_attach needs igraph and glib and is not built here.  The results of
the sample are checked equal between the two before anything is written.

  python tools/attach_time.py [--out profiles/attach_c4shape.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "shadow-1_amd"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--vertices", type=int, default=100_000)
    ap.add_argument("--hosts", type=int, default=16_384)
    ap.add_argument("--sample", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=1.0, help="timed window of the batched call")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attach_c4shape.json"))
    args = ap.parse_args()
    import numpy as np
    from shdpe import engine as E
    from shdpe import generators as G

    va = G.vertex_attrs(args.vertices, seed=4, n_city=200, n_country=60, n_geo=6, n_type=3)
    hints = G.attach_hints(va, args.hosts, seed=5)
    at = E.Attacher(va)                      # raises without a gfx950 device: no fallback
    out = at.attach(hints)                   # warm-up: code object load, staging buffers
    kernel, wall = [], []
    t_end = time.perf_counter() + args.seconds
    while time.perf_counter() < t_end or len(kernel) < 5:
        t0 = time.perf_counter()
        out = at.attach(hints)
        wall.append((time.perf_counter() - t0) * 1e3)
        kernel.append(at.timing()["kernel_ms"])
    at.close()

    idx = np.linspace(0, args.hosts - 1, args.sample).astype(np.int64)
    sample = {k: np.ascontiguousarray(v[idx]) for k, v in hints.items()}
    E.attach_host(va, sample, 0)             # warm-up
    t0 = time.perf_counter()
    host = [E.attach_host(va, sample, i) for i in range(args.sample)]
    host_ms = (time.perf_counter() - t0) * 1e3
    for j, i in enumerate(idx):
        for k, v in host[j].items():
            if out[k][i].item() != v:
                raise SystemExit(f"host {i}: {k} differs between the batched call and the host loop")
    host_scaled = host_ms * args.hosts / args.sample

    cs = out["candidate_set"].astype(int)
    res = {
        "vertices": args.vertices, "hosts": args.hosts, "unit": "ms",
        "batched_calls_timed": len(kernel),
        "batched_kernel_ms": {"median": statistics.median(kernel), "min": min(kernel), "max": max(kernel)},
        "batched_wall_ms": {"median": statistics.median(wall), "min": min(wall), "max": max(wall)},
        "host_loop_sample_hosts": args.sample, "host_loop_sample_ms": host_ms,
        "host_loop_scaled_ms": host_scaled,
        "host_loop_over_batched_wall": host_scaled / statistics.median(wall),
        "host_loop_over_batched_kernel": host_scaled / statistics.median(kernel),
        "compared_against": "shd_pe_attach_host (one query per call, one thread) on the same box; "
                            "Shadow's topology_attach itself needs igraph / glib and is not built here",
        "hosts_per_candidate_set": {str(s): int((cs == s).sum()) for s in range(9)},
        "hosts_longest_prefix": int((out["used_random"] == 0).sum()),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
