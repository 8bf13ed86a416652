"""Price a batch plan on the CPU: the engine's own planner (pe_plan.cpp through
tools/sim/plan_capi.cpp) makes the batches of a config for batch orders 1 and
2, tools/sim/batch_sim.c counts every batch's arc visits with the kernel's
settings (dirty lanes, eager far set, delta = 0.75 x mean arc latency, hub
offsets), and the dynamic longest-first take is replayed over the counts.

Per order: mean arc visits per arc, the correlation of the planner's predicted
cost with the simulated visits, and the replay's makespan over the ideal
(total / P) at P = 256 (relax) and P = 512 (post) workgroups.

usage: python tools/sim/plan_eval.py [c4] [--batches N] [--procs P] [--fit] [--offsets] [--json OUT]
  --batches N   simulate an evenly spaced sample of N batches (default: all)
  --fit         also print the least-squares fit of order 2's visits on
                (1, mean offset, spread): batch_order_cost's constants
  --offsets     price order 2's batches under both lane offset kinds side by
                side (lane_offsets: 0 nearest hub, 1 least squares): visits
                per kind, their ratio per batch, and the take replayed in
                either kind's sequence
"""
import argparse
import ctypes
import heapq
import json
import multiprocessing as mp
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "shadow-1_amd"), HERE]
from shdpe import generators as G  # noqa: E402
from run_sim import Out, lib as sim_lib  # noqa: E402

LB = 16
P = ctypes.c_void_p


def plan_lib(build_dir=HERE):
    so = os.path.join(build_dir, "libplan.so")
    csrc = os.path.join(ROOT, "shadow-1_amd", "csrc")
    srcs = [os.path.join(HERE, "plan_capi.cpp"), os.path.join(csrc, "pe_plan.cpp"), os.path.join(csrc, "pe_graph.cpp")]
    deps = srcs + [os.path.join(csrc, "pe_plan.hpp"), os.path.join(csrc, "pe_graph.hpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-pthread", "-I", csrc,
                        "-I", os.path.join(ROOT, "include")] + srcs + ["-o", so], check=True)
    L = ctypes.CDLL(so)
    L.plan_create.restype = P
    L.plan_create.argtypes = [ctypes.c_int32, ctypes.c_int64, ctypes.c_int, P, P, P, P, P, ctypes.c_int32, ctypes.c_int]
    L.plan_destroy.argtypes = [P]
    L.plan_positions.argtypes = [P]
    L.plan_arcs.restype = ctypes.c_int64
    L.plan_arcs.argtypes = [P]
    L.plan_mean_arc_latency.restype = ctypes.c_double
    L.plan_mean_arc_latency.argtypes = [P]
    L.plan_csr.argtypes = [P, P, P, P]
    L.plan_batches.argtypes = [P, ctypes.c_int, P, P, P, P]
    L.plan_offset_kind.argtypes = [P, ctypes.c_int]
    L.plan_residual_spread.argtypes = [P, P]
    return L


def ptr(a):
    return a.ctypes.data_as(P)


def make_plan(L, top, att, order, kind=1, lanes=LB):
    """The planner's batches of the whole table with the lane offsets of
    `kind`, and the kernel's graph."""
    LB = lanes
    att = np.ascontiguousarray(att, np.int32)
    h = L.plan_create(top.n, top.m, int(top.directed), ptr(top.src), ptr(top.dst), ptr(top.latency),
                      ptr(top.loss), ptr(att), att.shape[0], order)
    assert h, "build_host_graph failed"
    L.plan_offset_kind(h, kind)
    T, m = L.plan_positions(h), L.plan_arcs(h)
    rp, col, lat = np.empty(top.n + 1, np.int32), np.empty(m, np.int32), np.empty(m, np.float64)
    L.plan_csr(h, ptr(rp), ptr(col), ptr(lat))
    nB = (T + LB - 1) // LB
    srcs, offs = np.empty(nB * LB, np.int32), np.empty(nB * LB, np.float64)
    cost, feat = np.empty(nB, np.float64), np.empty(2 * nB, np.float64)
    assert L.plan_batches(h, LB, ptr(srcs), ptr(offs), ptr(cost), ptr(feat)) == nB
    resid = np.empty(nB, np.float64)
    L.plan_residual_spread(h, ptr(resid))
    plan = dict(n=top.n, rp=rp, col=col, lat=lat, delta=0.75 * L.plan_mean_arc_latency(h), lanes=LB, resid=resid,
                unit=L.plan_mean_arc_latency(h),
                srcs=srcs.reshape(nB, LB), offs=offs.reshape(nB, LB), cost=cost, feat=feat.reshape(nB, 2))
    L.plan_destroy(h)
    return plan


_plan = None


def sim_batches(S, pl, idx):
    """Arc visits of the batches idx of the plan, with the kernel's settings."""
    arcs = np.empty(len(idx))
    for i, b in enumerate(idx):
        out = Out()
        s, o = np.ascontiguousarray(pl["srcs"][b]), np.ascontiguousarray(pl["offs"][b])
        rc = S.batch_sim(ctypes.c_int32(pl["n"]), ptr(pl["rp"]), ptr(pl["col"]), ptr(pl["lat"]), ptr(s), ptr(o),
                         ctypes.c_int32(1), ctypes.c_int32(pl["lanes"]), ctypes.c_double(pl["delta"]),
                         ctypes.c_int32(64), ctypes.c_int32(1), ctypes.c_int32(3), ctypes.byref(out), None)
        assert rc == 0
        arcs[i] = out.arcs
    return arcs


def _sim_batches(idx):
    """... of the worker's plan (inherited by fork)."""
    return sim_batches(sim_lib(), _plan, idx)


def simulate(plan, idx, procs):
    global _plan
    _plan = plan
    chunks = [c for c in np.array_split(idx, max(1, min(len(idx), procs * 8))) if len(c)]
    with mp.get_context("fork").Pool(procs) as pool:
        return np.concatenate(pool.map(_sim_batches, chunks)) / plan["col"].shape[0]


def same_batches(a, b):
    """For every batch of plan a its index in plan b: the two hold the same
    batches (the composition does not depend on the offsets), each in the
    sequence of its own predicted costs."""
    at = {tuple(r): i for i, r in enumerate(b["srcs"].tolist())}
    return np.array([at[tuple(r)] for r in a["srcs"].tolist()])


def price_offsets(L, top, att, sim, lanes=LB, batches=0):
    """Order 2's batches under both offset kinds.  sim(plan, idx) -> visits per
    arc.  Per kind the plan and the visits of its batches idx (kind 1's
    sequence; kind 0's are the same batches, found by same_batches)."""
    p1, p0 = make_plan(L, top, att, 2, 1, lanes), make_plan(L, top, att, 2, 0, lanes)
    nB = p1["cost"].shape[0]
    idx = np.arange(nB) if not batches or batches >= nB else np.unique(np.linspace(0, nB - 1, batches).astype(int))
    in0 = same_batches(p1, p0)
    return dict(idx=idx, in0=in0, plan1=p1, plan0=p0, arcs1=sim(p1, idx), arcs0=sim(p0, in0[idx]))


def offsets_report(pr):
    """The side-by-side figures of price_offsets' result."""
    a0, a1, idx, p0, p1 = pr["arcs0"], pr["arcs1"], pr["idx"], pr["plan0"], pr["plan1"]
    nB = p1["cost"].shape[0]
    ratio = a1 / a0
    top4 = np.argsort(-a0)[:max(1, len(a0) // 4)]
    r = {"batches": int(nB), "simulated": int(len(idx)),
         "nearest_hub_visits_per_m": float(a0.mean()), "least_squares_visits_per_m": float(a1.mean()),
         "ratio": float(a1.mean() / a0.mean()),
         "max_nearest_hub": float(a0.max()), "max_least_squares": float(a1.max()),
         "rel_sd_nearest_hub": float(a0.std() / a0.mean()), "rel_sd_least_squares": float(a1.std() / a1.mean()),
         "costliest_quarter_ratio": float(a1[top4].sum() / a0[top4].sum()),
         "batches_worse": int((ratio > 1.0).sum()), "worst_batch_ratio": float(ratio.max()),
         "corr_cost_nearest_hub": float(np.corrcoef(p0["cost"][pr["in0"][idx]], a0)[0, 1]),
         "corr_cost_least_squares": float(np.corrcoef(p1["cost"][idx], a1)[0, 1]),
         "corr_mean_hub_distance": float(np.corrcoef(p1["feat"][idx, 0], a1)[0, 1]),
         "corr_spread": float(np.corrcoef(p1["feat"][idx, 1], a1)[0, 1]),
         "corr_residual_spread": float(np.corrcoef(p1["resid"][idx], a1)[0, 1])}
    real = p1["srcs"][idx] >= 0
    meanNew = (p1["offs"][idx] * real).sum(axis=1) / real.sum(axis=1) / p1["unit"]
    r["corr_mean_lane_offset"] = float(np.corrcoef(meanNew, a1)[0, 1]) if meanNew.std() > 0 else 0.0
    # the refit: (1, mean nearest-hub distance, residual spread) on kind 1's visits
    X = np.column_stack([np.ones(len(idx)), p1["feat"][idx, 0], p1["resid"][idx]])
    coef, *_ = np.linalg.lstsq(X, a1, rcond=None)
    r["fit_c0_off_spread"] = [float(c) for c in coef]
    r["fit_corr"] = float(np.corrcoef(X @ coef, a1)[0, 1])
    if len(idx) == nB:
        seq0 = np.argsort(pr["in0"])            # kind 1's batch indices in kind 0's sequence
        refit = np.argsort(-(X @ coef), kind="stable")
        for w in (256, 512):
            ideal0, ideal1 = a0.sum() / w, a1.sum() / w
            r[f"P{w}"] = {
                "nearest_hub_makespan": makespan(a0[seq0], w),
                "least_squares_makespan_old_sequence": makespan(a1[seq0], w),
                "least_squares_makespan": makespan(a1, w),
                "least_squares_makespan_refit": makespan(a1[refit], w),
                "least_squares_makespan_by_true_cost": makespan(np.sort(a1)[::-1], w),
                "nearest_hub_over_ideal": makespan(a0[seq0], w) / ideal0,
                "old_sequence_over_ideal": makespan(a1[seq0], w) / ideal1,
                "over_ideal": makespan(a1, w) / ideal1,
                "refit_over_ideal": makespan(a1[refit], w) / ideal1,
                "by_true_cost_over_ideal": makespan(np.sort(a1)[::-1], w) / ideal1}
    return r


def makespan(costs, workers):
    """Workgroups take the batches in sequence, each when it falls idle."""
    h = [0.0] * workers
    for c in costs:
        heapq.heappush(h, heapq.heappop(h) + c)
    return max(h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", nargs="?", default="c4")
    ap.add_argument("--batches", type=int, default=0)
    ap.add_argument("--procs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--fit", action="store_true")
    ap.add_argument("--offsets", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    top, att = G.make_config(args.workload)
    L = plan_lib()
    sim_lib()                      # compiled before the workers fork
    res = {"workload": args.workload, "lanes": LB, "orders": {}}
    if args.offsets:
        pr = price_offsets(L, top, att, lambda plan, idx: simulate(plan, idx, args.procs), LB, args.batches)
        res["lane_offsets"] = offsets_report(pr)
        print("lane offsets: " + json.dumps(res["lane_offsets"]), flush=True)
    for order in () if args.offsets else (1, 2):
        plan = make_plan(L, top, att, order)
        nB = plan["cost"].shape[0]
        idx = np.arange(nB) if not args.batches or args.batches >= nB else \
            np.unique(np.linspace(0, nB - 1, args.batches).astype(int))
        arcs = simulate(plan, idx, args.procs)
        r = {"batches": int(nB), "simulated": int(len(idx)), "arc_visits_per_m_mean": float(arcs.mean()),
             "arc_visits_per_m_min": float(arcs.min()), "arc_visits_per_m_max": float(arcs.max()),
             "arc_visits_per_m_sd": float(arcs.std()),
             "corr_predicted_cost": float(np.corrcoef(plan["cost"][idx], arcs)[0, 1]),
             "corr_mean_offset": float(np.corrcoef(plan["feat"][idx, 0], arcs)[0, 1]),
             "corr_spread": float(np.corrcoef(plan["feat"][idx, 1], arcs)[0, 1])}
        if len(idx) == nB:
            # (the batches are in the planner's take sequence already)
            for workers in (256, 512):
                r[f"makespan_P{workers}"] = makespan(arcs, workers)
                r[f"makespan_over_ideal_P{workers}"] = makespan(arcs, workers) / (arcs.sum() / workers)
                r[f"makespan_by_true_cost_P{workers}"] = makespan(np.sort(arcs)[::-1], workers)
        if args.fit and order == 2:
            X = np.column_stack([np.ones(len(idx)), plan["feat"][idx, 0], plan["feat"][idx, 1]])
            coef, *_ = np.linalg.lstsq(X, arcs, rcond=None)
            r["fit_c0_off_spread"] = [float(c) for c in coef]
            r["fit_corr"] = float(np.corrcoef(X @ coef, arcs)[0, 1])
        res["orders"][str(order)] = r
        print(f"order {order}: " + json.dumps(r), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
