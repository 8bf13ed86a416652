// The create-time planning of pe_plan.cpp (degree_order, relabel_graph,
// batch_ranks, batch_order, select_mode, batch_round_size, shd_pe_plan_shards)
// over graphs that tests/test_host.py writes as raw arrays (batch_round_size
// takes plain numbers: its cases are in the code): a graph directory holds meta.txt
// ("n directed hasVloss"), from.i32, to.i32, lat.f64, loss.f64, vloss.f64 and
// att.i32 (the attached list); the HostGraph comes from build_host_graph.
// Built with pe_plan.cpp and pe_graph.cpp, -fsanitize=address,undefined; no HIP.
//
//   plan DIR...             every check on every graph, "OK" when all hold
//   plan --fixture OUT DIR  degree_order, both orders' ranks and offsets and
//                           batch_order (LB 8, 16) of DIR as text, doubles as
//                           their bit patterns (tests/golden/host_plan_ba1200.txt)
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <queue>
#include <random>
#include <string>
#include <vector>

#include "pe_graph.hpp"
#include "pe_plan.hpp"

using namespace shdpe;

namespace {

int failures = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) { if (++failures <= 20) std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); } \
    } while (0)

template <class T>
std::vector<T> read_array(const std::string& path) {
    std::vector<T> v;
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) { std::printf("cannot read %s\n", path.c_str()); std::exit(2); }
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)bytes / sizeof(T));
    if (!v.empty() && std::fread(v.data(), sizeof(T), v.size(), f) != v.size()) std::exit(2);
    std::fclose(f);
    return v;
}

struct Case {
    HostGraph g;
    std::vector<int32_t> attached, posOf;   // unique attached, vertex -> position or -1
};

void set_attached(Case& c, const std::vector<int32_t>& att) {
    c.attached.clear();
    c.posOf.assign(c.g.n, -1);
    for (int32_t v : att)
        if (c.posOf[v] < 0) { c.posOf[v] = (int32_t)c.attached.size(); c.attached.push_back(v); }
}

Case load(const std::string& dir) {
    int n = 0, directed = 0, hasVloss = 0;
    FILE* f = std::fopen((dir + "/meta.txt").c_str(), "r");
    if (!f || std::fscanf(f, "%d %d %d", &n, &directed, &hasVloss) != 3) {
        std::printf("cannot read %s/meta.txt\n", dir.c_str());
        std::exit(2);
    }
    std::fclose(f);
    const auto from = read_array<int32_t>(dir + "/from.i32"), to = read_array<int32_t>(dir + "/to.i32");
    const auto lat = read_array<double>(dir + "/lat.f64"), loss = read_array<double>(dir + "/loss.f64");
    const auto vloss = hasVloss ? read_array<double>(dir + "/vloss.f64") : std::vector<double>();
    ShdPeGraphDesc d{n, (int64_t)from.size(), directed, from.data(), to.data(), lat.data(), loss.data(),
                     hasVloss ? vloss.data() : nullptr};
    Case c;
    if (build_host_graph(&d, &c.g) != SHD_PE_OK) { std::printf("build_host_graph failed: %s\n", dir.c_str()); std::exit(2); }
    set_attached(c, read_array<int32_t>(dir + "/att.i32"));
    return c;
}

template <class V>
bool same_bytes(const V& a, const V& b) {
    return a.size() == b.size() &&
           (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(a[0])) == 0);
}
bool same_bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

int32_t degree(const HostGraph& g, int32_t v) { return g.rowPtr[v + 1] - g.rowPtr[v]; }

void test_degree_order(const HostGraph& g) {
    const std::vector<int32_t> od = degree_order(g);
    CHECK((int32_t)od.size() == g.n);
    std::vector<uint8_t> seen(g.n, 0);
    for (int32_t v : od) { CHECK(v >= 0 && v < g.n && !seen[v]); seen[v] = 1; }
    for (int32_t k = 1; k < g.n; ++k) {
        CHECK(degree(g, od[k - 1]) >= degree(g, od[k]));
        if (degree(g, od[k - 1]) == degree(g, od[k])) CHECK(od[k - 1] < od[k]);
    }
}

// a plain Dijkstra over the OUT rows (no findArc: valid on a relabelled graph)
std::vector<double> dijkstra(const HostGraph& g, int32_t s) {
    std::vector<double> dist(g.n, INFINITY);
    typedef std::pair<double, int32_t> QE;
    std::priority_queue<QE, std::vector<QE>, std::greater<QE>> q;
    dist[s] = 0.0;
    q.push({0.0, s});
    while (!q.empty()) {
        const QE top = q.top();
        q.pop();
        if (top.first > dist[top.second]) continue;
        for (int32_t a = g.rowPtr[top.second]; a < g.rowPtr[top.second + 1]; ++a) {
            const double nd = top.first + g.lat[a];
            if (nd < dist[g.col[a]]) { dist[g.col[a]] = nd; q.push({nd, g.col[a]}); }
        }
    }
    return dist;
}

// r = relabel_graph(g, oldOf): vertex k of r is vertex oldOf[k] of g
void check_relabel(const HostGraph& g, const std::vector<int32_t>& oldOf) {
    const HostGraph r = relabel_graph(g, oldOf);
    const int32_t n = g.n;
    std::vector<int32_t> newOf(n);
    for (int32_t k = 0; k < n; ++k) newOf[oldOf[k]] = k;
    CHECK(r.n == n && r.directed == g.directed && r.nEdges == g.nEdges && r.latFold == g.latFold);
    CHECK(r.isComplete == g.isComplete && same_bits(r.meanArcLatency, g.meanArcLatency) &&
          same_bits(r.minArcLatency, g.minArcLatency));
    CHECK(r.nArcs() == g.nArcs() && (int32_t)r.rowPtr.size() == n + 1 && r.rowPtr[0] == 0);
    CHECK(r.lat.size() == r.col.size() && r.rel.size() == r.col.size() && r.outToIn.size() == r.col.size());
    CHECK(r.foldLat.size() == (g.latFold ? r.col.size() : 0) && r.selfPathRel.size() == r.foldLat.size());
    // OUT rows: the original row arc for arc, targets renamed, the values' bits
    for (int32_t k = 0; k < n; ++k) {
        const int32_t u = oldOf[k];
        CHECK(degree(r, k) == degree(g, u));
        if (degree(r, k) != degree(g, u)) return;
        for (int32_t a = g.rowPtr[u], j = r.rowPtr[k]; a < g.rowPtr[u + 1]; ++a, ++j) {
            CHECK(r.col[j] == newOf[g.col[a]] && oldOf[r.col[j]] == g.col[a]);
            CHECK(same_bits(r.lat[j], g.lat[a]) && same_bits(r.rel[j], g.rel[a]));
            if (g.latFold)
                CHECK(same_bits(r.foldLat[j], g.foldLat[a]) && same_bits(r.selfPathRel[j], g.selfPathRel[a]));
        }
    }
    // IN rows (directed; an undirected graph has none on either side)
    if (g.directed) {
        CHECK((int32_t)r.inPtr.size() == n + 1 && r.inCol.size() == r.col.size() &&
              r.inLat.size() == r.col.size() && r.inRel.size() == r.col.size());
        for (int32_t k = 0; k < n; ++k) {
            const int32_t v = oldOf[k];
            CHECK(r.inPtr[k + 1] - r.inPtr[k] == g.inPtr[v + 1] - g.inPtr[v]);
            if (r.inPtr[k + 1] - r.inPtr[k] != g.inPtr[v + 1] - g.inPtr[v]) return;
            for (int32_t a = g.inPtr[v], j = r.inPtr[k]; a < g.inPtr[v + 1]; ++a, ++j) {
                CHECK(r.inCol[j] == newOf[g.inCol[a]]);
                CHECK(same_bits(r.inLat[j], g.inLat[a]) && same_bits(r.inRel[j], g.inRel[a]));
            }
        }
    } else {
        CHECK(r.inPtr.empty() && r.inCol.empty() && r.inLat.empty() && r.inRel.empty());
    }
    // outToIn: arc k -> c points at the in-arc of c that comes from k, same latency
    const std::vector<int32_t>& ip = g.directed ? r.inPtr : r.rowPtr;
    const hvec<int32_t>& ic = g.directed ? r.inCol : r.col;
    const hvec<double>& il = g.directed ? r.inLat : r.lat;
    for (int32_t k = 0; k < n; ++k)
        for (int32_t j = r.rowPtr[k]; j < r.rowPtr[k + 1]; ++j) {
            const int32_t c = r.col[j], i = r.outToIn[j];
            CHECK(i >= ip[c] && i < ip[c + 1]);
            if (i >= ip[c] && i < ip[c + 1]) CHECK(ic[i] == k && same_bits(il[i], r.lat[j]));
        }
    // per-vertex arrays
    CHECK(r.edgeCount.size() == g.edgeCount.size());
    for (int32_t k = 0; k < n; ++k) {
        const int32_t v = oldOf[k];
        CHECK(same_bits(r.vrel[k], g.vrel[v]) && same_bits(r.selfLat[k], g.selfLat[v]) &&
              same_bits(r.selfRel[k], g.selfRel[v]) && same_bits(r.selfMinLat[k], g.selfMinLat[v]) &&
              same_bits(r.selfMinRel[k], g.selfMinRel[v]) && r.hasSelf[k] == g.hasSelf[v]);
        if (!g.edgeCount.empty()) CHECK(r.edgeCount[k] == g.edgeCount[v]);
    }
    // distances from five sources: vertex for vertex, and so as a multiset
    for (int i = 0; i < 5; ++i) {
        const int32_t s = (int32_t)((int64_t)(n - 1) * i / 4);
        std::vector<double> dg = dijkstra(g, s), dr = dijkstra(r, newOf[s]);
        bool same = true;
        for (int32_t v = 0; v < n; ++v) same = same && same_bits(dg[v], dr[newOf[v]]);
        CHECK(same);
        std::sort(dg.begin(), dg.end());
        std::sort(dr.begin(), dr.end());
        CHECK(same_bytes(dg, dr));
    }
}

void test_relabel(const HostGraph& g) {
    check_relabel(g, degree_order(g));
    std::vector<int32_t> perm(g.n);
    for (int32_t v = 0; v < g.n; ++v) perm[v] = v;
    const std::vector<int32_t> identity = perm;
    std::mt19937 rng(12345u + (unsigned)g.n);
    std::shuffle(perm.begin(), perm.end(), rng);
    check_relabel(g, perm);
    check_relabel(g, identity);
    const HostGraph r = relabel_graph(g, identity);
    CHECK(r.rowPtr == g.rowPtr && same_bytes(r.col, g.col) && same_bytes(r.lat, g.lat) && same_bytes(r.rel, g.rel));
    CHECK(r.inPtr == g.inPtr && same_bytes(r.inCol, g.inCol) && same_bytes(r.inLat, g.inLat) &&
          same_bytes(r.inRel, g.inRel) && same_bytes(r.outToIn, g.outToIn));
    CHECK(same_bytes(r.foldLat, g.foldLat) && same_bytes(r.selfPathRel, g.selfPathRel));
    CHECK(same_bytes(r.vrel, g.vrel) && same_bytes(r.selfLat, g.selfLat) && same_bytes(r.selfRel, g.selfRel) &&
          same_bytes(r.selfMinLat, g.selfMinLat) && same_bytes(r.selfMinRel, g.selfMinRel) &&
          r.hasSelf == g.hasSelf && r.edgeCount == g.edgeCount);
}

void check_batch_order(const BatchRanks& br, int LB, const std::vector<int32_t>& pos) {
    const int32_t T = (int32_t)br.rank.size(), cnt = (int32_t)pos.size();
    int32_t nB = -1;
    const std::vector<int32_t> order = batch_order(br.rank, br.rowOff, LB, pos.data(), cnt, nB);
    CHECK(nB == (cnt + LB - 1) / LB && order.size() == (size_t)nB * LB);
    if (order.size() != (size_t)nB * LB) return;
    // every position once, the rest pads
    std::vector<int> want(T, 0), got(T, 0);
    for (int32_t p : pos) want[p]++;
    size_t pads = 0;
    for (int32_t p : order) {
        CHECK(p >= -1 && p < T);
        if (p >= 0 && p < T) got[p]++; else ++pads;
    }
    CHECK(want == got && pads == order.size() - (size_t)cnt);
    // in a batch: ascending rank, pads only behind the rows; batches: in rank
    // order without offsets, in non-increasing mean offset with them
    std::vector<double> mean(nB, 0.0);
    for (int32_t b = 0; b < nB; ++b) {
        int c = 0;
        double s = 0.0;
        for (int l = 0; l < LB; ++l) {
            const int32_t p = order[(size_t)b * LB + l];
            if (p < 0) continue;
            CHECK(c == l);
            if (l > 0 && c == l) CHECK(br.rank[order[(size_t)b * LB + l - 1]] < br.rank[p]);
            if (!br.rowOff.empty()) s += br.rowOff[p];
            ++c;
        }
        CHECK(c > 0);
        mean[b] = c ? s / c : 0.0;
        if (b > 0 && !br.rowOff.empty()) CHECK(mean[b - 1] >= mean[b]);
        if (b > 0 && br.rowOff.empty()) CHECK(br.rank[order[(size_t)b * LB - 1]] < br.rank[order[(size_t)b * LB]]);
    }
}

// equal ranks keep the order of pos[] (the sort by rank is stable)
void test_batch_order_ties() {
    BatchRanks br;
    br.rank = {1, 0, 1, 0, 1, 0, 0, 1, 1, 0, 2};
    const std::vector<int32_t> pos = {10, 8, 2, 4, 0, 9, 5, 3, 1};
    int32_t nB = 0;
    const std::vector<int32_t> order = batch_order(br.rank, br.rowOff, 4, pos.data(), (int32_t)pos.size(), nB);
    CHECK(nB == 3 && (order == std::vector<int32_t>{9, 5, 3, 1, 8, 2, 4, 0, 10, -1, -1, -1}));
}

void check_ranks(const Case& c) {
    const HostGraph& g = c.g;
    const int32_t T = (int32_t)c.attached.size();
    const std::vector<int32_t> od = degree_order(g);
    const int32_t K = (int32_t)std::max<int64_t>(1, std::min<int64_t>(256, g.n / 400));
    for (int order = 0; order <= 1; ++order) {
        const BatchRanks br = batch_ranks(g, c.attached, c.posOf, order);
        CHECK((int32_t)br.rank.size() == T);
        std::vector<uint8_t> seen(T, 0);
        for (int32_t r : br.rank) {
            CHECK(r >= 0 && r < T && !seen[r]);
            if (r >= 0 && r < T) seen[r] = 1;
        }
        if (order == 0) {
            CHECK(br.rowOff.empty());
        } else {
            CHECK((int32_t)br.rowOff.size() == T);
            for (double d : br.rowOff) CHECK(std::isfinite(d) && d >= 0.0);
            for (int32_t k = 0; k < K; ++k)
                if (c.posOf[od[k]] >= 0) CHECK(br.rowOff[c.posOf[od[k]]] == 0.0);
        }
        // all positions (T no multiple of LB), a subset, and a single batch
        std::vector<int32_t> all(T), third, few;
        for (int32_t p = 0; p < T; ++p) all[p] = T - 1 - p;
        for (int32_t p = 0; p < T; p += 3) third.push_back(p);
        for (int32_t p = 0; p < std::min(T, 5); ++p) few.push_back((p * 7) % T);
        std::sort(few.begin(), few.end());
        few.erase(std::unique(few.begin(), few.end()), few.end());
        for (int LB : {8, 16}) {
            check_batch_order(br, LB, all);
            check_batch_order(br, LB, third);
            check_batch_order(br, LB, few);
        }
    }
}

void test_ranks(Case c) {
    CHECK(c.attached.size() % 16 != 0 && c.attached.size() % 8 != 0);
    check_ranks(c);
    // every vertex attached: the hubs are among them (offset 0)
    std::vector<int32_t> all(c.g.n);
    for (int32_t v = 0; v < c.g.n; ++v) all[v] = c.g.n - 1 - v;
    set_attached(c, all);
    check_ranks(c);
}

HostGraph small_graph(int32_t n, bool complete) {
    std::vector<int32_t> from, to;
    for (int32_t v = 0; v < n; ++v) {
        from.push_back(v); to.push_back(v);
        for (int32_t u = complete ? 0 : v; u < v; ++u) { from.push_back(v); to.push_back(u); }
        if (!complete) { from.push_back(v); to.push_back((v + 1) % n); }
    }
    const std::vector<double> lat(from.size(), 2.0), loss(from.size(), 0.0);
    ShdPeGraphDesc d{n, (int64_t)from.size(), 0, from.data(), to.data(), lat.data(), loss.data(), nullptr};
    HostGraph g;
    CHECK(build_host_graph(&d, &g) == SHD_PE_OK);
    return g;
}

// forceMode 0..5 -> mode, per graph kind and density threshold
void test_select_mode() {
    const HostGraph ring = small_graph(40, false), full = small_graph(6, true), big = small_graph(65537, false);
    CHECK(!ring.isComplete && full.isComplete && !big.isComplete);
    const double ringDensity = (double)ring.nArcs() / (40.0 * 40.0);
    struct Row { const HostGraph* g; double denseMin; int mode[6]; };
    const Row table[] = {
        {&ring, 0.25, {1, 1, 2, 1, 3, 1}},          // sparse: SSSP rows unless forced
        {&ring, ringDensity, {3, 1, 2, 1, 3, 1}},   // at the threshold: dense, forceMode 0 only
        {&full, 0.25, {2, 1, 2, 1, 3, 1}},          // complete: direct rows
        {&full, 0.0, {2, 1, 2, 1, 3, 1}},
        {&big, 0.0, {1, 1, 2, 1, 1, 1}},            // past 65,536 vertices: never dense
    };
    for (const Row& r : table)
        for (int f = 0; f < 6; ++f) CHECK(select_mode(*r.g, f, r.denseMin) == r.mode[f]);
}

void test_plan_shards() {
    int32_t b[9];
    CHECK(shd_pe_plan_shards(-1, 1, 1, b) == SHD_PE_EINVAL && shd_pe_plan_shards(1, 0, 1, b) == SHD_PE_EINVAL &&
          shd_pe_plan_shards(1, 1, 0, b) == SHD_PE_EINVAL && shd_pe_plan_shards(1, 1, 1, nullptr) == SHD_PE_EINVAL);
    CHECK(shd_pe_plan_shards(16384, 8, 16, b) == SHD_PE_OK);
    for (int g = 0; g <= 8; ++g) CHECK(b[g] == 2048 * g);
    CHECK(shd_pe_plan_shards(100, 3, 16, b) == SHD_PE_OK);
    CHECK(b[0] == 0 && b[1] == 32 && b[2] == 64 && b[3] == 100);
    CHECK(shd_pe_plan_shards(0, 2, 16, b) == SHD_PE_OK && b[0] == 0 && b[2] == 0);
}

// batch_round_size: the batches per round of the split batch kernels, from the
// free device memory (ensure_batch passes hipMemGetInfo's figure)
void test_batch_round_size() {
    const size_t GiB = (size_t)1 << 30, GB = 1000000000;
    const size_t reserve = ROUND_RESERVE_BYTES, distCap = ROUND_DIST_CAP_BYTES;
    CHECK(reserve == 12 * GiB && distCap == 160 * GiB);
    // no room (free memory at or below rest + 12 GiB, or below rest alone): max(slots, 1)
    const size_t perD = 50 * 1000 * 1000, rest = 3 * GiB;
    for (size_t freeB : {(size_t)0, rest - 1, rest, rest + 1, rest + reserve - 1, rest + reserve})
        for (size_t slots : {(size_t)0, (size_t)1, (size_t)7, (size_t)512}) {
            CHECK(batch_round_size(slots, 4096, perD, rest, freeB, 0) == std::max<size_t>(slots, 1));
            CHECK(batch_round_size(slots, 4096, perD, rest, freeB, 3) == std::max<size_t>(slots, 1));
        }
    // one byte past it is still one batch; room for k arrays is k batches
    CHECK(batch_round_size(1, 4096, perD, rest, rest + reserve + 1, 0) == 1);
    CHECK(batch_round_size(1, 4096, perD, rest, rest + reserve + 2 * perD - 1, 0) == 1);
    CHECK(batch_round_size(1, 4096, perD, rest, rest + reserve + 2 * perD, 0) == 2);
    CHECK(batch_round_size(1, 4096, perD, rest, rest + reserve + 100 * perD + 17, 0) == 100);
    // never below slots; never above nBatchesAll (slots <= nBatchesAll); every batch when all fit
    std::mt19937_64 rng(77);
    for (int i = 0; i < 20000; ++i) {
        const size_t nAll = 1 + rng() % 70000, slots = 1 + rng() % std::min<size_t>(nAll, 2048);
        const size_t pd = 64 * 8 + rng() % (4 * GiB), rs = rng() % (64 * GiB), fr = rng() % (300 * GiB);
        const int cap = (int)(rng() % 4 == 0 ? 0 : rng() % 3000);
        const size_t r0 = batch_round_size(slots, nAll, pd, rs, fr, 0), rc = batch_round_size(slots, nAll, pd, rs, fr, cap);
        CHECK(slots <= nAll);
        CHECK(r0 >= slots && r0 <= nAll && rc >= slots && rc <= nAll);
        // the round's distance arrays fit the room and the cap, unless the slots force more
        if (r0 > slots) CHECK(r0 * pd <= distCap && r0 * pd + rs + reserve <= fr);
        if (r0 < nAll) CHECK((r0 + 1) * pd > distCap || (r0 + 1) * pd + rs + reserve > fr);
        // the test cap bounds from above only, and not below the slots
        CHECK(rc <= r0);
        if (cap > 0) CHECK(rc == std::max(slots, std::min(r0, (size_t)cap)));
        else CHECK(rc == r0);
    }
    CHECK(batch_round_size(4, 40, perD, rest, 200 * GiB, 0) == 40);
    CHECK(batch_round_size(4, 40, perD, rest, 200 * GiB, 1000) == 40);   // (a cap above: unchanged)
    CHECK(batch_round_size(4, 40, perD, rest, 200 * GiB, 5) == 5);
    CHECK(batch_round_size(4, 40, perD, rest, 200 * GiB, 4) == 4);
    CHECK(batch_round_size(4, 40, perD, rest, 200 * GiB, 1) == 4);       // (not below the slots)
    CHECK(batch_round_size(4, 40, perD, rest, 200 * GiB, -1) == 40);
    // the 160 GiB cap: 1 GiB arrays, 1 TiB free
    CHECK(batch_round_size(1, 4096, GiB, 0, 1024 * GiB, 0) == 160);
    CHECK(batch_round_size(1, 4096, GiB + 1, 0, 1024 * GiB, 0) == 159);
    CHECK(batch_round_size(256, 4096, GiB, 0, 1024 * GiB, 0) == 256);   // (the slots stand above it)
    // C4: 16,384 rows at 16 lanes = 1,024 batches, 13 GB of distance arrays; C5: 131 GB in
    // 4,096 batches beside a 107 GB table on a 288 GB card -- one round each
    CHECK(batch_round_size(1024, 1024, 13 * GB / 1024, 26 * GB, 250 * GiB, 0) == 1024);
    CHECK(batch_round_size(512, 4096, 131 * GB / 4096 + 1, 33 * GB, 288 * GB - 107 * GB, 0) == 4096);
    // ... and C5 under a 96 GiB budget would be two: the cap is what keeps it at one
    CHECK(96 * GiB / (131 * GB / 4096 + 1) < 4096);
    // near 2^40 bytes: no product or sum wraps
    const size_t T = (size_t)1 << 40;
    CHECK(batch_round_size(1, 1000000, T, T, 4 * T, 0) == 1);            // (one array is past the cap)
    CHECK(batch_round_size(1, 1000000, 16 * GiB, T, 4 * T, 0) == 10);
    CHECK(batch_round_size(3, 1000000, T - 1, T - 1, T, 0) == 3);
    CHECK(batch_round_size(2, (size_t)1 << 31, 512, 3 * T, 4 * T, 0) == 160 * GiB / 512);
    CHECK(batch_round_size(1, 8, 512, SIZE_MAX - 5, SIZE_MAX, 0) == 1);  // (rest + 12 GiB would wrap)
    CHECK(batch_round_size(1, 8, 0, 0, 64 * GiB, 0) == 8);               // (no vertex)
}

void put_ints(FILE* f, const char* name, const std::vector<int32_t>& v) {
    std::fprintf(f, "%s %zu\n", name, v.size());
    for (size_t i = 0; i < v.size(); ++i) std::fprintf(f, "%d%c", v[i], (i + 1) % 16 == 0 || i + 1 == v.size() ? '\n' : ' ');
}
void put_doubles(FILE* f, const char* name, const std::vector<double>& v) {
    std::fprintf(f, "%s %zu\n", name, v.size());
    for (size_t i = 0; i < v.size(); ++i) {
        unsigned long long bits;
        std::memcpy(&bits, &v[i], 8);
        std::fprintf(f, "%016llx%c", bits, (i + 1) % 6 == 0 || i + 1 == v.size() ? '\n' : ' ');
    }
}

int write_fixture(const char* out, const Case& c) {
    FILE* f = std::fopen(out, "w");
    if (!f) return 2;
    put_ints(f, "degree_order", degree_order(c.g));
    std::vector<int32_t> pos(c.attached.size());
    for (size_t p = 0; p < pos.size(); ++p) pos[p] = (int32_t)p;
    for (int order = 0; order <= 1; ++order) {
        const BatchRanks br = batch_ranks(c.g, c.attached, c.posOf, order);
        put_ints(f, order ? "rank_order1" : "rank_order0", br.rank);
        put_doubles(f, order ? "rowOff_order1" : "rowOff_order0", br.rowOff);
        for (int LB : {8, 16}) {
            int32_t nB = 0;
            const std::string name = "batch_order" + std::to_string(order) + "_lb" + std::to_string(LB);
            put_ints(f, name.c_str(), batch_order(br.rank, br.rowOff, LB, pos.data(), (int32_t)pos.size(), nB));
        }
    }
    return std::fclose(f) == 0 ? 0 : 2;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 4 && std::strcmp(argv[1], "--fixture") == 0) return write_fixture(argv[2], load(argv[3]));
    if (argc < 2) { std::printf("usage: plan DIR... | plan --fixture OUT DIR\n"); return 2; }
    for (int i = 1; i < argc; ++i) {
        const Case c = load(argv[i]);
        test_degree_order(c.g);
        test_relabel(c.g);
        test_ranks(c);
        std::printf("%s: n %d arcs %lld directed %d latFold %d attached %zu\n", argv[i], c.g.n,
                    (long long)c.g.nArcs(), c.g.directed, (int)c.g.latFold, c.attached.size());
    }
    test_batch_order_ties();
    test_select_mode();
    test_plan_shards();
    test_batch_round_size();
    if (failures) return 1;
    std::printf("OK\n");
    return 0;
}
