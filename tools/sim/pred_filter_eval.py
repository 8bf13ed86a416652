"""Predecessor filter on the CPU simulator: how many of the in-arcs the post
kernel's on-demand predecessor pass reads are flagged by the relax (some active
lane's pre-check of the arc found du + w <= dist[x]), and that the flags are a
superset of the tight in-arcs.

The plan and graph are the engine's own (pe_plan.cpp through plan_capi.cpp,
batch order 2), the relax is tools/sim/batch_sim.c with the kernel's settings
(dirty lanes, eager far set, delta = 0.75 x mean arc latency, hub offsets).
Per batch, as fractions of the m arcs: the in-arcs of the vertices the pass
claims (the targets and, round by round, every lane's tree parents), those of
them that are flagged, those that are tight in some lane.  Asserts that every
arc tight in any lane is flagged and that no unflagged arc undercuts its head.

usage: python tools/sim/pred_filter_eval.py [c4] [--batches 6] [--lanes 16]
"""
import argparse
import ctypes
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "shadow-1_amd"), HERE]
from run_sim import Out  # noqa: E402

P = ctypes.c_void_p


def ptr(a):
    return a.ctypes.data_as(P)


def sim_lib(build_dir=HERE):
    so = os.path.join(build_dir, "batch_sim.so")
    src = os.path.join(HERE, "batch_sim.c")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.run(["gcc", "-O3", "-shared", "-fPIC", src, "-o", so, "-lm"], check=True)
    S = ctypes.CDLL(so)
    S.sim_set_flags.argtypes = [P, P]
    return S


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
    return L


def make_plan(L, top, att, lanes, order=2):
    """The planner's batches of the whole table at `lanes` sources per batch,
    and the kernel's graph (out-arc CSR in the device's vertex ids)."""
    att = np.ascontiguousarray(att, np.int32)
    h = L.plan_create(top.n, top.m, int(top.directed), ptr(top.src), ptr(top.dst), ptr(top.latency),
                      ptr(top.loss), ptr(att), att.shape[0], order)
    assert h, "build_host_graph failed"
    T, m = L.plan_positions(h), L.plan_arcs(h)
    rp, col, lat = np.empty(top.n + 1, np.int32), np.empty(m, np.int32), np.empty(m, np.float64)
    L.plan_csr(h, ptr(rp), ptr(col), ptr(lat))
    nB = (T + lanes - 1) // lanes
    srcs, offs = np.empty(nB * lanes, np.int32), np.empty(nB * lanes, np.float64)
    cost, feat = np.empty(nB, np.float64), np.empty(2 * nB, np.float64)
    assert L.plan_batches(h, lanes, ptr(srcs), ptr(offs), ptr(cost), ptr(feat)) == nB
    plan = dict(n=top.n, rp=rp, col=col, lat=lat, delta=0.75 * L.plan_mean_arc_latency(h), lanes=lanes,
                srcs=srcs.reshape(nB, lanes), offs=offs.reshape(nB, lanes),
                tail=np.repeat(np.arange(top.n, dtype=np.int32), np.diff(rp)))
    L.plan_destroy(h)
    return plan


def relax_batch(S, plan, b):
    """Batch b on the simulator: (flag byte per out-arc, final distances [n][lanes])."""
    n, lanes = plan["n"], plan["lanes"]
    flag = np.zeros(plan["col"].shape[0], np.uint8)
    D = np.empty((n, lanes), np.float64)
    out = Out()
    s, o = np.ascontiguousarray(plan["srcs"][b]), np.ascontiguousarray(plan["offs"][b])
    S.sim_set_flags(ptr(flag), ptr(D))
    try:
        rc = S.batch_sim(ctypes.c_int32(n), ptr(plan["rp"]), ptr(plan["col"]), ptr(plan["lat"]), ptr(s), ptr(o),
                         ctypes.c_int32(1), ctypes.c_int32(lanes), ctypes.c_double(plan["delta"]),
                         ctypes.c_int32(64), ctypes.c_int32(1), ctypes.c_int32(3), ctypes.byref(out), None)
    finally:
        S.sim_set_flags(None, None)
    assert rc == 0
    return flag, D


def arc_classes(plan, D):
    """Per out-arc u -> x over the final distances: tight in some lane
    (D[u] + w == D[x], finite), undercutting its head in some lane."""
    cand = D[plan["tail"]] + plan["lat"][:, None]
    dx = D[plan["col"]]
    fin = np.isfinite(cand)
    return (fin & (cand == dx)).any(axis=1), (cand < dx).any(axis=1)


def claimed_vertices(plan, D, b):
    """The vertices the on-demand pass claims: the targets, then round by round
    the tree parents (tight in-arc of minimum dist[u]) of the claimed vertices
    in every lane."""
    n, lanes = plan["n"], plan["lanes"]
    tail, head, w = plan["tail"], plan["col"], plan["lat"]
    du = D[tail]
    tight = np.isfinite(du) & (du + w[:, None] == D[head])
    key = np.where(tight, du, np.inf)
    best = np.full((n, lanes), np.inf)
    np.minimum.at(best, head, key)
    parent = np.full((n, lanes), -1, np.int64)
    isbest = tight & (key == best[head])
    a_idx, l_idx = np.nonzero(isbest)
    parent[head[a_idx], l_idx] = tail[a_idx]
    srcs = plan["srcs"][b]
    for l, s in enumerate(srcs):
        if s >= 0:
            parent[s, l] = -1
    claimed = np.zeros(n, bool)
    targets = np.unique(plan["srcs"][plan["srcs"] >= 0])
    new = targets
    while new.size:
        claimed[new] = True
        par = parent[new][:, srcs >= 0].ravel()
        par = np.unique(par[par >= 0])
        new = par[~claimed[par]]
    return claimed


def batch_row(S, plan, b):
    flag, D = relax_batch(S, plan, b)
    tight, under = arc_classes(plan, D)
    assert not (tight & (flag == 0)).any(), f"batch {b}: a tight arc is not flagged"
    assert not (under & (flag == 0)).any(), f"batch {b}: an unflagged arc undercuts its head"
    assert not under.any(), f"batch {b}: the relax left a Bellman violation"
    claimed = claimed_vertices(plan, D, b)
    inarc = claimed[plan["col"]]
    m = float(plan["col"].shape[0])
    return dict(batch=int(b), claimed_vertices=claimed.sum() / plan["n"], in_arcs=inarc.sum() / m,
                flagged=(inarc & (flag != 0)).sum() / m, tight=(inarc & tight).sum() / m)


def main():
    from shdpe import generators as G
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", nargs="?", default="c4")
    ap.add_argument("--batches", type=int, default=6)
    ap.add_argument("--lanes", type=int, default=16)
    args = ap.parse_args()
    top, att = G.make_config(args.workload)
    plan = make_plan(plan_lib(), top, att, args.lanes)
    S = sim_lib()
    nB = plan["srcs"].shape[0]
    print("| batch | claimed vertices | in-arcs of claimed vertices | of those, flagged | of those, tight in some lane |")
    print("|---|---|---|---|---|")
    for b in np.unique(np.linspace(5, nB - 9, args.batches).astype(int)):
        r = batch_row(S, plan, b)
        print(f"| {r['batch']} | {r['claimed_vertices']:.3f} of n | {r['in_arcs']:.3f} | {r['flagged']:.3f} | "
              f"{r['tight']:.3f} |", flush=True)


if __name__ == "__main__":
    main()
