"""Time of the graph property check (shd_pe_graph_props, the device form,
against shd_pe_graph_props_host, the host form of this repository) at three
shapes a user runs:

  c4    power-law graph, 100,000 vertices (generators.power_law(100_000, m=3, seed=4))
  c5    power-law graph, 250,000 vertices (generators.power_law(250_000, m=2, seed=6))
  c3a   complete graph on 20,000 vertices with self-loops: 2.0001e8 edges
        grouped by source, as a GraphML writer lists them

Per shape, after one warm-up call of each form, device and host calls
alternate until the device calls fill the window (at least 3 of each); the
device call reports usCall (wall, upload included) and usDevice (events
around its kernels), the host call is timed with a host clock.  The answers
of the two forms are compared before anything is written.  At c3a the two
k_props_count forms alternate as well (SHDPE_PROPS_COUNT=plain is the
one-atomic-per-edge kernel); their usDevice differs by that kernel alone.

The sweep-budget probe is a directed graph of c5's vertex and edge counts
that never converges within its budget (a ring over all vertices, the other
edges parallel ring arcs: the pivot's reach advances one arc per sweep):
usDevice / sweeps of a call that exhausts a budget of 2,048 is the cost of one
sweep at that size, host reads included.  The default budget follows as
(host form's time at c5) / (that cost): past it the host form would have
answered sooner.

The comparison point is this repository's host form on the same box: the
reference's igraph calls need igraph and are not built here, so they are not
timed.

  python tools/props_time.py [--out profiles/graph_props.json] [--shapes c4,c5,c3a]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "shadow-1_amd"))


class Graph:
    def __init__(self, n, directed, src, dst):
        self.n, self.directed, self.src, self.dst = n, directed, src, dst
        self.m = int(src.shape[0])


def make_shape(name, c3_n):
    import numpy as np
    from shdpe import generators as G
    if name == "c4":
        t = G.power_law(100_000, m=3, seed=4)
        return Graph(t.n, False, t.src, t.dst)
    if name == "c5":
        t = G.power_law(250_000, m=2, seed=6)
        return Graph(t.n, False, t.src, t.dst)
    if name == "c3a":                                    # generators.dense's edges without its 2e8 latencies
        iu, ju = G._triu_pairs(c3_n)
        loops = np.arange(c3_n, dtype=np.int32)
        return Graph(c3_n, False, np.concatenate([iu, loops]), np.concatenate([ju, loops]))
    raise KeyError(name)


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


FIELDS = ("isDirected", "isConnected", "clusterCount", "largestCluster", "isComplete", "firstIncomplete")


def time_shape(E, g, seconds, count_forms):
    import numpy as np
    forms = ("runs", "plain") if count_forms else ("runs",)
    dev = {f: {"usCall": [], "usDevice": []} for f in forms}
    host_ms = []

    def device(form):
        os.environ["SHDPE_PROPS_COUNT"] = form
        return E.graph_props(g, device=0, membership=True)

    def host():
        t0 = time.perf_counter()
        r = E.graph_props(g, membership=True)
        return r, (time.perf_counter() - t0) * 1e3

    ref, _ = host()                                      # warm-up of both forms, and the comparison
    for f in forms:
        d = device(f)
        if d["info"]["handedOff"]:
            raise SystemExit(f"{f}: the device form handed off: {d['info']}")
        for k in FIELDS:
            if d[k] != ref[k]:
                raise SystemExit(f"{f}: {k} differs between the device and the host form")
        if not np.array_equal(d["membership"], ref["membership"]):
            raise SystemExit(f"{f}: membership differs between the device and the host form")
    info = d["info"]
    spent = 0.0
    while spent < seconds or len(host_ms) < 3:
        for f in forms:
            i = device(f)["info"]
            dev[f]["usCall"].append(i["usCall"])
            dev[f]["usDevice"].append(i["usDevice"])
            spent += i["usCall"] * 1e-6
        host_ms.append(host()[1])
    os.environ.pop("SHDPE_PROPS_COUNT", None)
    res = {"vertices": g.n, "edges": g.m, "directed": bool(g.directed),
           "props": {k: ref[k] for k in FIELDS},
           "sweeps": info["sweeps"], "rounds": info["rounds"],
           "device_calls_timed": len(dev["runs"]["usCall"]),
           "device_usCall": spread(dev["runs"]["usCall"]), "device_usDevice": spread(dev["runs"]["usDevice"]),
           "host_calls_timed": len(host_ms), "host_ms": spread(host_ms)}
    res["host_over_device_call"] = res["host_ms"]["median"] * 1e3 / res["device_usCall"]["median"]
    if count_forms:
        res["count_plain_usCall"] = spread(dev["plain"]["usCall"])
        res["count_plain_usDevice"] = spread(dev["plain"]["usDevice"])
        res["count_runs_usDevice"] = res["device_usDevice"]
    return res


def budget_probe(E, like, budget=2048, calls=5):
    """usDevice per sweep of a directed graph with `like`'s counts that
    exhausts `budget` (module docstring)."""
    import numpy as np
    ring = np.arange(like.n, dtype=np.int32)
    extra = np.arange(like.m - like.n, dtype=np.int64) % like.n
    src = np.concatenate([ring, extra.astype(np.int32)])
    g = Graph(like.n, True, src, (src + 1) % like.n)
    # the host form takes over after the hand-off and is not what is timed here
    per = []
    for i in range(calls + 1):
        info = E.graph_props(g, device=0, sweep_budget=budget)["info"]
        if not info["handedOff"] or info["sweeps"] != budget:
            raise SystemExit(f"probe: expected a hand-off at {budget} sweeps, got {info}")
        if i:
            per.append(info["usDevice"] / info["sweeps"])
    return {"vertices": g.n, "edges": g.m, "budget": budget, "calls": calls, "us_per_sweep": spread(per)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="c4,c5,c3a")
    ap.add_argument("--c3-n", type=int, default=20_000)
    ap.add_argument("--seconds", type=float, default=1.0, help="timed window of the device calls per shape")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_props.json"))
    args = ap.parse_args()
    from shdpe import engine as E

    res = {"unit": "usCall / usDevice in microseconds, host_ms in milliseconds",
           "compared_against": "shd_pe_graph_props_host (one thread) on the same box, alternating with the "
                               "device form; the reference's igraph_is_connected / igraph_clusters / "
                               "_topology_isComplete need igraph and are not built here: not measured",
           "shapes": {}}
    for name in args.shapes.split(","):
        g = make_shape(name, args.c3_n)
        res["shapes"][name] = time_shape(E, g, args.seconds, count_forms=(name == "c3a"))
        print(name, json.dumps(res["shapes"][name]), flush=True)
        if name == "c5":
            p = budget_probe(E, g)
            host_us = res["shapes"]["c5"]["host_ms"]["median"] * 1e3
            p["host_form_us_at_c5"] = host_us
            p["sweeps_at_which_device_time_passes_host_form"] = host_us / p["us_per_sweep"]["median"]
            res["sweep_budget_probe"] = p
            print("probe", json.dumps(p), flush=True)
        del g
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
