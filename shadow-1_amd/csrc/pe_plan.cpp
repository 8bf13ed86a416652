// pe_plan.cpp -- create-time planning of the engine (pure C++, no HIP); see
// pe_plan.hpp.
#include "pe_plan.hpp"

#include <algorithm>
#include <atomic>
#include <climits>
#include <cmath>
#include <functional>
#include <queue>
#include <system_error>
#include <thread>
#include <utility>

namespace shdpe {

std::vector<int32_t> degree_order(const HostGraph& g) {
    std::vector<int32_t> oldOf(g.n);
    for (int32_t v = 0; v < g.n; ++v) oldOf[v] = v;
    std::stable_sort(oldOf.begin(), oldOf.end(), [&](int32_t a, int32_t b) {
        return g.rowPtr[a + 1] - g.rowPtr[a] > g.rowPtr[b + 1] - g.rowPtr[b];
    });
    return oldOf;
}

// rows[k] = the row of oldOf[k]: the row pointers, and per old arc its new index
static std::vector<int32_t> permute_rows(const std::vector<int32_t>& ptr, const std::vector<int32_t>& oldOf,
                                         std::vector<int32_t>& arcNew) {
    const int32_t n = (int32_t)oldOf.size();
    std::vector<int32_t> np(n + 1, 0);
    arcNew.resize(ptr[n]);
    for (int32_t k = 0; k < n; ++k) {
        const int32_t u = oldOf[k];
        np[k + 1] = np[k] + (ptr[u + 1] - ptr[u]);
        for (int32_t a = ptr[u], j = np[k]; a < ptr[u + 1]; ++a, ++j) arcNew[a] = j;
    }
    return np;
}

template <class V>
static void permute(V& dst, const V& src, const std::vector<int32_t>& newIdx) {
    dst.resize(src.size());
    for (size_t a = 0; a < src.size(); ++a) dst[newIdx[a]] = src[a];
}

HostGraph relabel_graph(const HostGraph& g, const std::vector<int32_t>& oldOf) {
    const int32_t n = g.n;
    const size_t m = (size_t)g.nArcs();
    HostGraph r;
    r.n = n; r.directed = g.directed; r.nEdges = g.nEdges;
    r.latFold = g.latFold; r.isComplete = g.isComplete;
    r.meanArcLatency = g.meanArcLatency; r.minArcLatency = g.minArcLatency;
    std::vector<int32_t> newOf(n);
    for (int32_t k = 0; k < n; ++k) newOf[oldOf[k]] = k;
    std::vector<int32_t> arcNew, inNew;
    r.rowPtr = permute_rows(g.rowPtr, oldOf, arcNew);
    permute(r.lat, g.lat, arcNew);
    permute(r.rel, g.rel, arcNew);
    permute(r.foldLat, g.foldLat, arcNew);           // (empty unless latFold)
    permute(r.selfPathRel, g.selfPathRel, arcNew);
    r.col.resize(m);
    for (size_t a = 0; a < m; ++a) r.col[arcNew[a]] = newOf[g.col[a]];
    if (g.directed) {
        r.inPtr = permute_rows(g.inPtr, oldOf, inNew);
        permute(r.inLat, g.inLat, inNew);
        permute(r.inRel, g.inRel, inNew);
        r.inCol.resize(m);
        for (size_t a = 0; a < m; ++a) r.inCol[inNew[a]] = newOf[g.inCol[a]];
    }
    // (undirected: the in-arc of an arc is its reverse arc in the OUT arrays)
    const std::vector<int32_t>& revNew = g.directed ? inNew : arcNew;
    r.outToIn.resize(m);
    for (size_t a = 0; a < m; ++a) r.outToIn[arcNew[a]] = revNew[g.outToIn[a]];
    permute(r.vrel, g.vrel, newOf);
    permute(r.selfLat, g.selfLat, newOf);
    permute(r.selfRel, g.selfRel, newOf);
    permute(r.selfMinLat, g.selfMinLat, newOf);
    permute(r.selfMinRel, g.selfMinRel, newOf);
    permute(r.hasSelf, g.hasSelf, newOf);
    permute(r.edgeCount, g.edgeCount, newOf);        // (empty unless a multigraph)
    return r;
}

// Multi-source Dijkstra over the out-arcs from the hubs byDeg[first],
// byDeg[first + step], ... below K: every vertex's distance to its closest
// hub and that hub's rank (equal distances: the lower rank).
static void hub_dijkstra(const HostGraph& g, const std::vector<int32_t>& byDeg, int32_t first, int32_t step,
                         int32_t K, std::vector<double>& dist, std::vector<int32_t>& owner) {
    dist.assign(g.n, INFINITY);
    owner.assign(g.n, INT32_MAX);
    typedef std::pair<double, int32_t> QE;
    std::priority_queue<QE, std::vector<QE>, std::greater<QE>> q;
    for (int32_t k = first; k < K; k += step) { dist[byDeg[k]] = 0.0; owner[byDeg[k]] = k; q.push({0.0, byDeg[k]}); }
    while (!q.empty()) {
        const QE top = q.top();
        q.pop();
        const int32_t u = top.second;
        if (top.first > dist[u]) continue;
        for (int32_t a = g.rowPtr[u]; a < g.rowPtr[u + 1]; ++a) {
            const int32_t v = g.col[a];
            const double nd = dist[u] + g.lat[a];
            if (nd < dist[v] || (nd == dist[v] && owner[u] < owner[v])) {
                dist[v] = nd;
                owner[v] = owner[u];
                q.push({nd, v});
            }
        }
    }
}

static int32_t hub_count(const HostGraph& g) {
    return (int32_t)std::max<int64_t>(1, std::min<int64_t>(256, g.n / 400));
}

HubGroups hub_group_distances(const HostGraph& g, const std::vector<int32_t>& attached, int threads) {
    HubGroups out;
    out.G = HUB_GROUPS;
    const size_t T = attached.size();
    out.dist.assign(T * HUB_GROUPS, INFINITY);
    out.hub.assign(T * HUB_GROUPS, INT32_MAX);
    const int32_t K = hub_count(g);
    const int passes = (int)std::min<int32_t>(K, HUB_GROUPS);      // groups K.. are empty
    const std::vector<int32_t> byDeg = degree_order(g);
    if (threads <= 0) {
        const unsigned hw = std::thread::hardware_concurrency();
        threads = (int)std::min<unsigned>(16, hw ? hw : 1);
    }
    threads = std::max(1, std::min(threads, passes));
    // every thread takes the next pass: a pass has its own distance and owner
    // arrays and writes only its own column of the output, so who runs it
    // (and a thread that could not be started) changes nothing
    std::atomic<int> next{0};
    auto run = [&]() {
        std::vector<double> dist;
        std::vector<int32_t> owner;
        for (int j; (j = next.fetch_add(1)) < passes;) {
            hub_dijkstra(g, byDeg, j, HUB_GROUPS, K, dist, owner);
            for (size_t p = 0; p < T; ++p) {
                out.dist[p * HUB_GROUPS + j] = dist[attached[p]];
                out.hub[p * HUB_GROUPS + j] = owner[attached[p]];
            }
        }
    };
    std::vector<std::thread> pool;
    try {
        for (int t = 1; t < threads; ++t) pool.emplace_back(run);
    } catch (const std::system_error&) {
    }
    run();
    for (std::thread& th : pool) th.join();
    return out;
}

// Order 2: positions by (nearest hub, nearest hub of another group, the gap
// between their distances, the nearest's distance, position); sources that
// no hub reaches have hub INT32_MAX and so come last.
static void rank_by_hub_groups(BatchRanks& out, size_t T) {
    const HubGroups& hg = out.groups;
    struct Key { int32_t h1, h2; double gap, d1; int32_t p; };
    std::vector<Key> key(T);
    out.rowOff.assign(T, 0.0);
    for (size_t p = 0; p < T; ++p) {
        const double* d = &hg.dist[p * hg.G];
        const int32_t* h = &hg.hub[p * hg.G];
        int j1 = -1, j2 = -1;
        auto closer = [&](int a, int b) { return b < 0 || d[a] < d[b] || (d[a] == d[b] && h[a] < h[b]); };
        for (int j = 0; j < hg.G; ++j) {
            if (!std::isfinite(d[j])) continue;
            if (closer(j, j1)) { j2 = j1; j1 = j; }
            else if (closer(j, j2)) j2 = j;
        }
        Key& k = key[p];
        k.p = (int32_t)p;
        k.h1 = j1 >= 0 ? h[j1] : INT32_MAX;
        k.d1 = j1 >= 0 ? d[j1] : INFINITY;
        k.h2 = j2 >= 0 ? h[j2] : INT32_MAX;
        k.gap = j2 >= 0 ? d[j2] - d[j1] : INFINITY;
        if (j1 >= 0) out.rowOff[p] = d[j1];
    }
    std::sort(key.begin(), key.end(), [](const Key& a, const Key& b) {
        if (a.h1 != b.h1) return a.h1 < b.h1;
        if (a.h2 != b.h2) return a.h2 < b.h2;
        if (a.gap != b.gap) return a.gap < b.gap;
        if (a.d1 != b.d1) return a.d1 < b.d1;
        return a.p < b.p;
    });
    out.rank.assign(T, 0);
    for (size_t i = 0; i < T; ++i) out.rank[key[i].p] = (int32_t)i;
}

BatchRanks batch_ranks(const HostGraph& g, const std::vector<int32_t>& attached,
                       const std::vector<int32_t>& posOf, int batchOrder) {
    BatchRanks out;
    if (batchOrder == 2) {
        out.groups = hub_group_distances(g, attached);
        rank_by_hub_groups(out, attached.size());
        return out;
    }
    std::vector<int32_t> order;
    order.reserve(g.n);
    if (batchOrder == 1) {
        std::vector<double> dist;
        std::vector<int32_t> owner;
        hub_dijkstra(g, degree_order(g), 0, 1, hub_count(g), dist, owner);
        for (int32_t v = 0; v < g.n; ++v) order.push_back(v);
        std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
            return owner[a] != owner[b] ? owner[a] < owner[b] : dist[a] < dist[b];
        });
        // bucket key offsets: a source's distance to its hub, so the lanes of
        // a batch reach the vertices behind the hub in the same bucket
        out.rowOff.assign(attached.size(), 0.0);
        for (size_t p = 0; p < attached.size(); ++p) {
            const double d = dist[attached[p]];
            out.rowOff[p] = std::isfinite(d) ? d : 0.0;
        }
    } else {
        std::vector<uint8_t> seen(g.n, 0);
        for (int32_t r = 0; r < g.n; ++r) {
            if (seen[r]) continue;
            seen[r] = 1;
            size_t head = order.size();
            order.push_back(r);
            while (head < order.size()) {
                const int32_t u = order[head++];
                for (int32_t a = g.rowPtr[u]; a < g.rowPtr[u + 1]; ++a) {
                    const int32_t v = g.col[a];
                    if (!seen[v]) { seen[v] = 1; order.push_back(v); }
                }
                if (g.directed) {
                    for (int32_t a = g.inPtr[u]; a < g.inPtr[u + 1]; ++a) {
                        const int32_t v = g.inCol[a];
                        if (!seen[v]) { seen[v] = 1; order.push_back(v); }
                    }
                }
            }
        }
    }
    out.rank.assign(attached.size(), 0);
    int32_t k = 0;
    for (int32_t v : order)
        if (posOf[v] >= 0) out.rank[posOf[v]] = k++;
    return out;
}

// pos[] stably sorted by rank in rows of LB, -1 pads the last row
static std::vector<int32_t> compose_batches(const std::vector<int32_t>& rank, int LB, const int32_t* pos,
                                            int32_t cnt, int32_t& nB) {
    // (rank, index in pos[]) packed into one integer key, so the sort
    // compares no more than the keys themselves
    std::vector<uint64_t> key(cnt);
    for (int32_t i = 0; i < cnt; ++i)
        key[i] = (uint64_t)((uint32_t)rank[pos[i]] ^ 0x80000000u) << 32 | (uint32_t)i;
    std::sort(key.begin(), key.end());
    std::vector<int32_t> order(cnt);
    for (int32_t i = 0; i < cnt; ++i) order[i] = pos[(uint32_t)key[i]];
    nB = (cnt + LB - 1) / LB;
    order.resize((size_t)nB * LB, -1);
    return order;
}

// The batches of order[] in the sequence of the stably sorted key[] = (key, batch)
template <class T>
static void permute_batches(std::vector<T>& order, int LB, const std::vector<std::pair<double, int32_t>>& key) {
    std::vector<T> re(order.size());
    for (size_t i = 0; i < key.size(); ++i)
        std::copy(order.begin() + (size_t)key[i].second * LB,
                  order.begin() + (size_t)(key[i].second + 1) * LB, re.begin() + i * LB);
    order.swap(re);
}

static void sequence_batches(std::vector<int32_t>& order, int LB, std::vector<std::pair<double, int32_t>>& key) {
    std::stable_sort(key.begin(), key.end());
    permute_batches(order, LB, key);
}

std::vector<double> lane_offsets(const HubGroups& groups, const std::vector<double>& rowOff,
                                 const std::vector<int32_t>& order, int LB, int kind) {
    std::vector<double> off(order.size(), 0.0);
    const int G = groups.G;
    std::vector<double> S(LB);
    for (size_t b0 = 0; b0 + LB <= order.size(); b0 += LB) {
        const int32_t* row = &order[b0];
        // J: the groups that reach every real lane (ascending)
        int nJ = 0;
        std::fill(S.begin(), S.end(), 0.0);
        for (int j = 0; kind == 1 && j < G; ++j) {
            bool all = true;
            for (int l = 0; l < LB && all; ++l)
                all = row[l] < 0 || std::isfinite(groups.dist[(size_t)row[l] * G + j]);
            if (!all) continue;
            ++nJ;
            for (int l = 0; l < LB; ++l)
                if (row[l] >= 0) S[l] += groups.dist[(size_t)row[l] * G + j];
        }
        if (!nJ) {      // no common landmark (or kind 0): the nearest-hub distances
            for (int l = 0; l < LB; ++l)
                if (row[l] >= 0 && !rowOff.empty()) off[b0 + l] = rowOff[row[l]];
            continue;
        }
        double mn = INFINITY;
        for (int l = 0; l < LB; ++l)
            if (row[l] >= 0) mn = std::min(mn, S[l]);
        for (int l = 0; l < LB; ++l)
            if (row[l] >= 0) off[b0 + l] = (S[l] - mn) / nJ;
    }
    return off;
}

std::vector<int32_t> batch_order(const std::vector<int32_t>& rank, const std::vector<double>& rowOff,
                                 int LB, const int32_t* pos, int32_t cnt, int32_t& nB) {
    std::vector<int32_t> order = compose_batches(rank, LB, pos, cnt, nB);
    if (!rowOff.empty() && nB > 1) {
        // longest batches first (workgroups take batches in order, so the last round is
        // made of short ones): a batch's cost grows with its sources' mean distance to
        // their hub (tools/sim/: correlation 0.53 with arc visits at C4)
        std::vector<std::pair<double, int32_t>> key(nB);
        for (int32_t b = 0; b < nB; ++b) {
            double s = 0.0;
            int c = 0;
            for (int l = 0; l < LB; ++l) {
                const int32_t p = order[(size_t)b * LB + l];
                if (p >= 0) { s += rowOff[p]; ++c; }
            }
            key[b] = {c ? -s / c : 0.0, b};
        }
        sequence_batches(order, LB, key);
    }
    return order;
}

// Predicted arc visits of a batch in passes over the arcs, least-squares fit
// to tools/sim/batch_sim.c's count over the 1,024 order-2 batches of C4
// (tools/sim/plan_eval.py c4 --fit; profiles/batch_plan_cost_sim.json holds
// the fit and its correlation, 0.945).  Only the order of the costs is used.
// The features stay those of the nearest-hub distance under least-squares
// lane offsets too: with the spread taken as the residual those offsets leave
// and the constants refitted, the correlation is 0.942 and the replayed take
// ends where this sequence does (profiles/lane_offsets_sim.json).
// (COST_C0, COST_OFF, COST_SPREAD: pe_plan.hpp, shared with the device plan.)

std::vector<int32_t> batch_order_cost(const std::vector<int32_t>& rank, const std::vector<double>& rowOff,
                                      const HubGroups& groups, double meanArcLatency, int LB,
                                      const int32_t* pos, int32_t cnt, int32_t& nB, std::vector<double>* cost,
                                      std::vector<double>* laneOff, int offsetKind) {
    std::vector<int32_t> order = compose_batches(rank, LB, pos, cnt, nB);
    std::vector<double> offs = lane_offsets(groups, rowOff, order, LB, offsetKind);
    const double unit = meanArcLatency > 0.0 && std::isfinite(meanArcLatency) ? meanArcLatency : 1.0;
    const int G = groups.G;
    std::vector<std::pair<double, int32_t>> key(nB);
    std::vector<double> sum(G), sumSq(G);
    std::vector<int> cntOf(G);
    for (int32_t b = 0; b < nB; ++b) {
        std::fill(sum.begin(), sum.end(), 0.0);
        std::fill(sumSq.begin(), sumSq.end(), 0.0);
        std::fill(cntOf.begin(), cntOf.end(), 0);
        double off = 0.0;
        int lanes = 0;
        for (int l = 0; l < LB; ++l) {
            const int32_t p = order[(size_t)b * LB + l];
            if (p < 0) continue;
            ++lanes;
            off += rowOff[p];
            for (int j = 0; j < G; ++j) {
                const double d = groups.dist[(size_t)p * G + j];
                if (!std::isfinite(d)) continue;
                const double x = (d - rowOff[p]) / unit;
                sum[j] += x;
                sumSq[j] += x * x;
                ++cntOf[j];
            }
        }
        double var = 0.0;
        int terms = 0;
        for (int j = 0; j < G; ++j) {
            if (!cntOf[j]) continue;
            var += std::max(0.0, sumSq[j] - sum[j] * sum[j] / cntOf[j]);
            terms += cntOf[j];
        }
        const double spread = terms ? std::sqrt(var / terms) : 0.0;
        const double meanOff = lanes ? off / lanes / unit : 0.0;
        const double c = (COST_C0 + COST_OFF * meanOff + COST_SPREAD * spread) * lanes / LB;
        key[b] = {-c, b};
    }
    if (nB > 1) {
        sequence_batches(order, LB, key);
        permute_batches(offs, LB, key);
    }
    if (laneOff) laneOff->swap(offs);
    if (cost) {
        cost->resize(nB);
        for (int32_t b = 0; b < nB; ++b) (*cost)[b] = -key[b].first;
    }
    return order;
}

size_t batch_round_size(size_t slots, size_t nBatchesAll, size_t perD, size_t rest, size_t freeB, int testCap) {
    if (perD == 0) perD = 1;         // (no vertex: nothing is persisted)
    // (freeB - rest - reserve without a sum that could wrap)
    const bool roomy = freeB > rest && freeB - rest > ROUND_RESERVE_BYTES;
    const size_t room = roomy ? freeB - rest - ROUND_RESERVE_BYTES : perD;
    const size_t dBudget = std::min(room, ROUND_DIST_CAP_BYTES);
    size_t roundB = std::max(slots, std::min(nBatchesAll, dBudget / perD));
    if (testCap > 0) roundB = std::max(slots, std::min(roundB, (size_t)testCap));
    return roundB;
}

int select_mode(const HostGraph& g, int forceMode, double denseMin) {
    int mode = (g.isComplete && forceMode != 1 && forceMode != 3) ? 2 : 1;
    if (forceMode == 2) mode = 2;
    // dense non-complete graphs: blocked min-plus (K2)
    const double density = (double)g.nArcs() / ((double)g.n * (double)g.n);
    const bool fitsDense = (int64_t)g.n <= 65536;
    if (mode == 1 && forceMode == 0 && fitsDense && density >= denseMin) mode = 3;
    if (forceMode == 4 && fitsDense) mode = 3;
    if (forceMode == 5) mode = 1;
    return mode;
}

}  // namespace shdpe

// Row-shard plan: G contiguous position ranges with equal numbers of kernel
// work units (a unit = one batch of 16 rows in the batched sparse kernel,
// one row otherwise).  Per-unit cost is near-uniform for this path: every
// SSSP row settles all n vertices, every dense / direct row is n (T) wide
// (measured per-batch cycle spread in DESIGN.md §6), so equal units are the
// balanced split, and contiguous ranges let the all-gather land rows in
// place.  Host-only (no device), exported for the CPU tests.
extern "C" int shd_pe_plan_shards(int32_t T, int32_t G, int32_t unit, int32_t* bounds) {
    if (T < 0 || G < 1 || unit < 1 || !bounds) return SHD_PE_EINVAL;
    const int64_t units = ((int64_t)T + unit - 1) / unit;
    for (int g = 0; g < G; ++g)
        bounds[g] = (int32_t)std::min<int64_t>(T, (units * g / G) * unit);
    bounds[G] = T;
    return SHD_PE_OK;
}
