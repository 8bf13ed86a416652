"""Restatements of Shadow's attach rule for the attach tests (plain helper
module, no tests in here).

serial()      _topology_findAttachmentVertex as topology.c:2094-2369 writes it:
              one hook call per vertex in vertex order pushing to eight queues,
              the clears on the first exact IP match, the first non-empty
              queue, the bestMatch loop, the pops of the random branch.
order_free()  the same rule without any order-dependent step (numpy over the
              vertices), for cases too large for the Python loop.

Both take the vertex attributes as an engine.VertexAttrs and the hints as the
dict Attacher.attach takes, and return for host i the six result fields
(vertex, candidate_set, num_candidates, used_random, bw_down, bw_up).
"""
import math

import numpy as np

NONE, ANY, LOOPBACK = 0xFFFFFFFF, 0, 0x7F000001
FIELDS = ("vertex", "candidate_set", "num_candidates", "used_random", "bw_down", "bw_up")
N_COMBOS = 17          # sets 0..7 x {prefix, random} + the exact-IP set


def usable(x: int) -> bool:
    return x != NONE and x != ANY and x != LOOPBACK          # :2127, :2264


def c_round(x: float) -> int:
    """C round(): half away from zero (Python's round() is half to even)."""
    return int(math.floor(x + 0.5)) if x >= 0 else -int(math.floor(-x + 0.5))


def vertex_lists(va):
    """Per vertex (ip, vertexHasUsableIP, city, country, geo, type) as Python
    values (a None column = no such key: nothing found)."""
    n = va.n
    ip = va.ip.tolist() if va.ip is not None else [NONE] * n
    cols = [(a.tolist() if a is not None else [-1] * n)
            for a in (va.citycode, va.countrycode, va.geocode, va.type)]
    return n, ip, list(zip(ip, [usable(x) for x in ip], *cols))


def _bw(col, v):
    if col is None or math.isnan(col[v]):
        return 0
    return int(col[v])                                        # (guint64) :2402, :2408


def serial(va, hints, i, lists=None):
    n, vip, rows = lists or vertex_lists(va)
    ip_given = bool(hints["ip_given"][i])
    hint_ip = int(hints["ip"][i])
    hc, hk, hg, ht = (int(hints[k][i]) for k in ("citycode", "countrycode", "geocode", "type"))
    r = float(hints["random"][i])
    # :2255-2268 (g_new0: requestedIP stays 0 unless usable)
    req_usable, requested = False, 0
    if ip_given and usable(hint_ip):
        req_usable, requested = True, hint_ip
    q = [[] for _ in range(8)]      # cityAndType, city, countryAndType, country, geoAndType, geo, type, all
    num_ips = [0] * 8
    found_exact = False
    for v, (ip, has_ip, c, k, g, t) in enumerate(rows):       # the hook, :2094-2217
        # found (code >= 0), hint given (>= 0; -2 matches nothing), strings equal (:2117-2120)
        city_m = c == hc and c >= 0 and hc >= 0
        country_m = k == hk and k >= 0 and hk >= 0
        geo_m = g == hg and g >= 0 and hg >= 0
        type_m = t == ht and t >= 0 and ht >= 0
        if req_usable and has_ip and ip == requested:         # :2134-2154
            if not found_exact:
                for qq in q:
                    qq.clear()
            found_exact = True
            q[7].append(v)
            num_ips[7] += 1
        if found_exact:                                       # :2157
            continue
        q[7].append(v)
        num_ips[7] += has_ip
        if city_m:                                            # :2166-2214
            if type_m:
                q[0].append(v)
                num_ips[0] += has_ip
            q[1].append(v)
            num_ips[1] += has_ip
        if country_m:
            if type_m:
                q[2].append(v)
                num_ips[2] += has_ip
            q[3].append(v)
            num_ips[3] += has_ip
        if geo_m:
            if type_m:
                q[4].append(v)
                num_ips[4] += has_ip
            q[5].append(v)
            num_ips[5] += has_ip
        if type_m:
            q[6].append(v)
            num_ips[6] += has_ip
    for s in range(8):                                        # :2293-2317
        if q[s]:
            break
    if s < 7:
        use_prefix = req_usable and num_ips[s] > 0
    else:
        use_prefix = ip_given and num_ips[7] > 0
    cand = q[s]
    num = len(cand)
    assert num > 0
    if use_prefix and not found_exact:                        # :2324-2325, :2219-2246
        best_match, chosen = 0, -1
        while cand:
            v = cand.pop(0)
            match = (~(vip[v] ^ requested)) & 0xFFFFFFFF
            if match > best_match or best_match == 0:
                best_match, chosen = match, v
        used_random = 0
    else:                                                     # :2327-2333
        k = c_round((num - 1) * r)
        chosen = -1
        while k >= 0:
            chosen = cand.pop(0)
            k -= 1
        used_random = 1
    return dict(vertex=chosen, candidate_set=8 if found_exact else s, num_candidates=num,
                used_random=used_random, bw_down=_bw(va.bandwidth_down, chosen),
                bw_up=_bw(va.bandwidth_up, chosen))


def order_free(va, hints, i):
    n = va.n
    vip = va.ip if va.ip is not None else np.full(n, NONE, np.uint32)
    none = np.full(n, -1, np.int32)
    cols = [a if a is not None else none for a in (va.citycode, va.countrycode, va.geocode, va.type)]
    ip_given = bool(hints["ip_given"][i])
    hint_ip = int(hints["ip"][i])
    r = float(hints["random"][i])
    req_usable = ip_given and usable(hint_ip)
    requested = np.uint32(hint_ip if req_usable else 0)
    vusable = (vip != NONE) & (vip != ANY) & (vip != LOOPBACK)
    mC, mK, mG, mT = ((c >= 0) & (c == int(hints[k][i])) for c, k in
                      zip(cols, ("citycode", "countrycode", "geocode", "type")))
    exact = vusable & (vip == requested) if req_usable else np.zeros(n, bool)
    if exact.any():
        s, members, use_prefix = 8, exact, False
    else:
        sets = (mC & mT, mC, mK & mT, mK, mG & mT, mG, mT, np.ones(n, bool))
        s = next(k for k in range(8) if sets[k].any())
        members = sets[s]
        has_ip = bool((members & vusable).any())
        use_prefix = has_ip and (req_usable if s < 7 else ip_given)
    idx = np.flatnonzero(members)
    if use_prefix:
        match = ~(vip[idx] ^ requested)
        mx = match.max()
        chosen = int(idx[-1]) if mx == 0 else int(idx[np.argmax(match)])     # argmax: first maximum
    else:
        chosen = int(idx[c_round((len(idx) - 1) * r)])
    return dict(vertex=chosen, candidate_set=s, num_candidates=int(len(idx)),
                used_random=0 if use_prefix else 1, bw_down=_bw(va.bandwidth_down, chosen),
                bw_up=_bw(va.bandwidth_up, chosen))


def combo(res) -> int:
    """0..15: set * 2 + used_random for sets 0..7; 16: the exact-IP set."""
    return 16 if res["candidate_set"] == 8 else res["candidate_set"] * 2 + res["used_random"]


def combos_of(out: dict) -> set:
    """combo() over a dict of result arrays (Attacher.attach)."""
    cs, ur = np.asarray(out["candidate_set"]).astype(int), np.asarray(out["used_random"]).astype(int)
    return set(np.where(cs == 8, 16, cs * 2 + ur).tolist())


def crafted_cases():
    """(name, VertexAttrs, hints, expected vertex, expected set, expected
    used_random) for the edge cases both attach test files run."""
    from shdpe.engine import VertexAttrs
    from shdpe.generators import ip_raw

    def va_of(ips, types=None, n=None):
        n = n or len(ips)
        bw = np.arange(1, n + 1, dtype=np.float64)
        return VertexAttrs(n, np.array([ip_raw(s) for s in ips], np.uint32), None, None, None,
                           None if types is None else np.array(types, np.int32), bw * 10, bw * 7)

    def hint(ip=None, type_=-1, r=0.25):
        return dict(ip_given=[0 if ip is None else 1], ip=[NONE if ip is None else ip_raw(ip)],
                    citycode=[-1], countrycode=[-1], geocode=[-1], type=[type_], random=[r])

    comp = "254.253.252.251"          # ~1.2.3.4: match == 0
    out = []
    # every type-matching vertex has match 0: the last candidate wins
    out.append(("all_zero_last", va_of(["10.0.0.1", comp, "10.0.0.2", comp, comp, "8.8.8.8"], [1, 0, 1, 0, 0, 1]),
                hint("1.2.3.4", 0), 4, 6, 0))
    # zeros before a positive match: the first positive maximum wins
    out.append(("zeros_then_max", va_of([comp, comp, "1.2.3.5", "1.2.3.5", comp, "9.9.9.9"], [0] * 6),
                hint("1.2.3.4", 0), 2, 6, 0))
    # hint given but unusable, no other hint: set 7, longest prefix against 0
    # (~(ip ^ 0) = ~ip on the raw little-endian s_addr: 1.0.0.0 = 0x00000001 -> 0xfffffffe beats
    # 8.8.8.8 -> 0xf7f7f7f7 and 0.0.0.255 = 0xff000000 -> 0x00ffffff)
    out.append(("unusable_hint_all", va_of(["8.8.8.8", "0.0.0.255", "1.0.0.0", "1.0.0.0"]),
                hint("0.0.0.0"), 2, 7, 0))
    # the first (only) exact-IP match is the last vertex
    ips = ["10.0.0.1"] * 129 + ["10.9.9.9"]
    out.append(("exact_at_last", va_of(ips, [0] * 130), hint("10.9.9.9", 0, 0.9), 129, 8, 1))
    # randomDouble 0.5: numCandidates - 1 even (4 -> 2) and odd (3 -> round(1.5) = 2)
    out.append(("half_even", va_of(["0.0.0.0"] * 5), hint(None, -1, 0.5), 2, 7, 1))
    out.append(("half_odd", va_of(["0.0.0.0"] * 4), hint(None, -1, 0.5), 2, 7, 1))
    # ... and through a filtered set (type 0 at vertices 1, 3, 4, 6): ordinal round(1.5) = 2 -> vertex 4
    out.append(("half_odd_typed", va_of(["0.0.0.0"] * 7, [1, 0, 1, 0, 0, 1, 0]), hint(None, 0, 0.5), 4, 6, 1))
    # randomDouble 1.0: the last candidate
    out.append(("one_last", va_of(["0.0.0.0"] * 70, [0, 1] * 35), hint(None, 1, 1.0), 69, 6, 1))
    return out
