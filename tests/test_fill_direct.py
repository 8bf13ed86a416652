"""The store rule of shd_pe_fill_rowstore_ex (include/shd_pathengine.h), pinned
on the CPU: a numpy model of the image its pack kernel builds
(k_pack_rowstore, pe_aux.hip) is adopted by an empty row store and compared
with the host sequence the header defines --

  1. shd_rowstore_store_rows over rows 0..T-1 in position order, with the
     prefersDirectPaths adjacency when PREFER_DIRECT (P) is set;
  2. with DIRECT_PAIRS (D): shd_rowstore_store(isDirect=1) for every ordered
     pair (p, q), p outer, that topology.c:2019-2021 serves from the edge
     itself (complete graph, or P and adjacent) and whose edge exists

-- over a random table and a random adjacency matrix.  No device needed; the
GPU tests (test_gpu_fill_direct.py) compare the kernel with the same
sequence."""
import ctypes as C

import numpy as np
import pytest

from shdpe.engine import RowStore, F_NOEDGE, F_UNREACHABLE, load_library

S_STORED, S_DIRECT, S_REVERSED = 1, 2, 4


def _random_table(T, seed, directed):
    """8% failed entries, 30% missing diagonals (test_rowstore._random_table)."""
    rng = np.random.default_rng(seed)
    lat = rng.uniform(0.5, 50.0, (T, T))
    rel = rng.uniform(0.9, 1.0, (T, T))
    flags = np.zeros((T, T), np.uint8)
    flags[rng.random((T, T)) < 0.08] = F_UNREACHABLE
    if not directed:
        flags = np.maximum(flags, flags.T)
    d = rng.random(T) < 0.3
    flags[d, d] = F_NOEDGE                              # missing (s, s) self-loops
    return lat, rel, flags


def _random_adjacency(T, seed, directed, density):
    """adj[p, q] = an arc p -> q exists (p == q: a self-loop) with its direct
    path values; symmetric when undirected, asymmetric when directed."""
    rng = np.random.default_rng(seed)
    adj = rng.random((T, T)) < density
    dlat = rng.uniform(0.1, 60.0, (T, T))               # some below every table latency
    drel = rng.uniform(0.8, 1.0, (T, T))
    if not directed:
        iu = np.triu_indices(T, 1)
        for m in (adj, dlat, drel):
            m.T[iu] = m[iu]
    return adj, dlat, drel


def fill_image_model(lat, rel, flags, adj, dlat, drel, complete, P, D):
    """The image of shd_pe_fill_rowstore_ex in numpy: per slot (a <= b) the
    first matching branch of
        forward fold ok and not (P and adj[a, b])            non-direct
        b > a, reverse fold ok and not (P and adj[b, a])     non-direct, REVERSED
        D and (P or complete) and adj[a, b]                  direct
        b > a, D and (P or complete) and adj[b, a]           direct, REVERSED
    where a complete graph takes no non-direct entry at all."""
    T = lat.shape[0]
    off = np.empty(T + 1, np.int64)
    assert load_library().shd_rowstore_image_layout(T, off.ctypes.data_as(C.c_void_p)) == 0
    img = np.zeros(int(off[T]), np.uint8)
    ok = (flags & (F_UNREACHABLE | F_NOEDGE)) == 0
    serveDirect = bool(D and (P or complete))
    stored, mn = 0, np.inf
    for a in range(T):
        n = T - a
        b = np.arange(a, T)
        up = b > a
        fwd = ok[a, b] & ~(P & adj[a, b]) & (not complete)
        rev = ~fwd & up & ok[b, a] & ~(P & adj[b, a]) & (not complete)
        dfw = ~fwd & ~rev & serveDirect & adj[a, b]
        drv = ~fwd & ~rev & ~dfw & up & serveDirect & adj[b, a]
        L = np.select([fwd, rev, dfw, drv], [lat[a, b], lat[b, a], dlat[a, b], dlat[b, a]], 0.0)
        R = np.select([fwd, rev, dfw, drv], [rel[a, b], rel[b, a], drel[a, b], drel[b, a]], 0.0)
        S = np.select([fwd, rev, dfw, drv], [S_STORED, S_STORED | S_REVERSED, S_STORED | S_DIRECT,
                                             S_STORED | S_DIRECT | S_REVERSED], 0).astype(np.uint8)
        o = int(off[a]) + 64
        img[o:o + 8 * n] = np.ascontiguousarray(L).view(np.uint8)
        img[o + 8 * n:o + 16 * n] = np.ascontiguousarray(R).view(np.uint8)
        img[o + 16 * n:o + 17 * n] = S
        stored += int((S != 0).sum())
        if (S != 0).any():
            mn = min(mn, float(L[S != 0].min()))
    return img, stored, (0.0 if stored == 0 else mn)


def host_sequence(ref, att, lat, rel, flags, adj, dlat, drel, complete, P, D):
    """The contract, with the existing host calls."""
    T = att.shape[0]
    rr = ref.store_rows(att, lat, rel, flags, is_complete=complete,
                        adjacent=np.ascontiguousarray(adj, dtype=np.uint8) if P else None)
    if D:
        for p in range(T):
            for q in range(T):
                if (complete or (P and adj[p, q])) and adj[p, q]:
                    ref.store(int(att[p]), int(att[q]), 1, int(complete), 0, dlat[p, q], drel[p, q])
    return rr


@pytest.mark.parametrize("complete", [False, True], ids=["incomplete", "complete"])
@pytest.mark.parametrize("D", [False, True], ids=["", "D"])
@pytest.mark.parametrize("P", [False, True], ids=["", "P"])
@pytest.mark.parametrize("directed", [False, True], ids=["undirected", "directed"])
def test_fill_rule_model_equals_host_sequence(directed, P, D, complete):
    T, n = 70, 90
    rng = np.random.default_rng(3)
    att = np.sort(rng.choice(n, size=T, replace=False)).astype(np.int32)
    lat, rel, flags = _random_table(T, 11 + int(directed), directed)
    # incomplete: a sparse adjacency; complete: every edge but a few (a
    # multigraph can pass _topology_isComplete with an edge missing)
    adj, dlat, drel = _random_adjacency(T, 5 + int(directed), directed, 0.97 if complete else 0.15)
    if directed:
        assert (adj != adj.T).sum() >= 100               # one-way arcs in both position orders
    assert adj.sum() >= 100 and adj.diagonal().any() and not adj.diagonal().all()
    ref = RowStore(n, att)
    host_sequence(ref, att, lat, rel, flags, adj, dlat, drel, complete, P, D)
    img, stored, mn = fill_image_model(lat, rel, flags, adj, dlat, drel, complete, P, D)
    st = RowStore(n, att)
    lib = load_library()
    REL = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p)
    keep = REL(lambda ctx, p: None)                     # the test owns the buffer
    assert lib.shd_rowstore_adopt_image(st.h, img.ctypes.data_as(C.c_void_p), img.nbytes,
                                        C.cast(keep, C.c_void_p), None, stored, mn) == 0
    assert st.size() == ref.size() == stored
    assert st.min_latency() == ref.min_latency()
    items = sorted(st.items())
    assert items == sorted(ref.items())
    for s in att:
        for d in att:
            assert st.get(int(s), int(d)) == ref.get(int(s), int(d)), (s, d)
    # what the flags mean, independent of either implementation
    pos = {int(v): i for i, v in enumerate(att)}
    direct = [e for e in items if e[4]]
    if not D or not (P or complete):
        assert not direct
    else:
        assert len(direct) >= 50
    for s, d, la, re_, isd, _ in items:
        p, q = pos[s], pos[d]
        if isd:
            assert adj[p, q] and (la, re_) == (dlat[p, q], drel[p, q])
        else:
            assert not complete and not (P and adj[p, q]) and (la, re_) == (lat[p, q], rel[p, q])
    if not P and not complete:
        # D alone changes nothing on an incomplete graph: today's fill
        plain = RowStore(n, att)
        plain.store_rows(att, lat, rel, flags)
        assert items == sorted(plain.items())
        plain.close()
    st.close()
    ref.close()
