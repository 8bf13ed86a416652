// Batch order 2 of pe_plan.cpp (hub_group_distances, batch_ranks order 2,
// batch_order_cost) over graphs that tests/test_plan_cost.py writes as raw
// arrays, in the layout of tests/native/plan.cpp's graph directories: meta.txt
// ("n directed hasVloss"), from.i32, to.i32, lat.f64, loss.f64, vloss.f64 and
// att.i32.  Built with pe_plan.cpp and pe_graph.cpp,
// -fsanitize=address,undefined; no HIP.
//
//   plan_cost DIR...    every check on every graph, "OK" when all hold
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <queue>
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
    c.posOf.assign(c.g.n, -1);
    for (int32_t v : read_array<int32_t>(dir + "/att.i32"))
        if (c.posOf[v] < 0) { c.posOf[v] = (int32_t)c.attached.size(); c.attached.push_back(v); }
    return c;
}

template <class V>
bool same_bytes(const V& a, const V& b) {
    return a.size() == b.size() &&
           (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(a[0])) == 0);
}
bool same_bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

// a plain Dijkstra over the out-arcs
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

// The group distances against one Dijkstra per hub, and for 1 and 16 threads.
HubGroups test_groups(const Case& c, int32_t K) {
    const int32_t T = (int32_t)c.attached.size();
    const HubGroups hg = hub_group_distances(c.g, c.attached, 1);
    CHECK(hg.G == HUB_GROUPS && hg.dist.size() == (size_t)T * hg.G && hg.hub.size() == hg.dist.size());
    if (hg.dist.size() != (size_t)T * HUB_GROUPS || hg.hub.size() != hg.dist.size()) return hg;
    for (int threads : {0, 2, 3, 16}) {
        const HubGroups o = hub_group_distances(c.g, c.attached, threads);
        CHECK(o.G == hg.G && same_bytes(o.dist, hg.dist) && same_bytes(o.hub, hg.hub));
    }
    const std::vector<int32_t> od = degree_order(c.g);
    std::vector<std::vector<double>> fromHub;
    for (int32_t k = 0; k < K; ++k) fromHub.push_back(dijkstra(c.g, od[k]));
    for (int32_t p = 0; p < T; ++p)
        for (int j = 0; j < hg.G; ++j) {
            double best = INFINITY;
            int32_t hub = INT32_MAX;
            for (int32_t k = j; k < K; k += hg.G)
                if (fromHub[k][c.attached[p]] < best) { best = fromHub[k][c.attached[p]]; hub = k; }
            CHECK(same_bits(hg.dist[(size_t)p * hg.G + j], best) && hg.hub[(size_t)p * hg.G + j] == hub);
        }
    return hg;
}

struct Key { int32_t h1, h2; double gap, d1; int32_t p; };

// (nearest hub, nearest hub of another group, gap, distance, position) of a
// position, by a scan of its own
Key key_of(const HubGroups& hg, int32_t p) {
    Key k{INT32_MAX, INT32_MAX, INFINITY, INFINITY, p};
    double d2 = INFINITY;
    int j1 = -1;
    for (int j = 0; j < hg.G; ++j) {
        const double d = hg.dist[(size_t)p * hg.G + j];
        const int32_t h = hg.hub[(size_t)p * hg.G + j];
        if (std::isfinite(d) && (d < k.d1 || (d == k.d1 && h < k.h1))) { k.d1 = d; k.h1 = h; j1 = j; }
    }
    for (int j = 0; j < hg.G; ++j) {
        const double d = hg.dist[(size_t)p * hg.G + j];
        const int32_t h = hg.hub[(size_t)p * hg.G + j];
        if (j != j1 && std::isfinite(d) && (d < d2 || (d == d2 && h < k.h2))) { d2 = d; k.h2 = h; }
    }
    if (k.h2 != INT32_MAX) k.gap = d2 - k.d1;
    return k;
}

bool key_less(const Key& a, const Key& b) {
    if (a.h1 != b.h1) return a.h1 < b.h1;
    if (a.h2 != b.h2) return a.h2 < b.h2;
    if (a.gap != b.gap) return a.gap < b.gap;
    if (a.d1 != b.d1) return a.d1 < b.d1;
    return a.p < b.p;
}

void check_cost_order(const BatchRanks& br, double unit, int LB, const std::vector<int32_t>& pos) {
    const int32_t T = (int32_t)br.rank.size(), cnt = (int32_t)pos.size();
    int32_t nB = -1, nB1 = -1;
    std::vector<double> cost;
    const std::vector<int32_t> order =
        batch_order_cost(br.rank, br.rowOff, br.groups, unit, LB, pos.data(), cnt, nB, &cost);
    CHECK(nB == (cnt + LB - 1) / LB && order.size() == (size_t)nB * LB && cost.size() == (size_t)nB);
    if (order.size() != (size_t)nB * LB || cost.size() != (size_t)nB) return;
    // every position once, the rest pads
    std::vector<int> want(T, 0), got(T, 0);
    for (int32_t p : pos) want[p]++;
    size_t pads = 0;
    for (int32_t p : order) {
        CHECK(p >= -1 && p < T);
        if (p >= 0 && p < T) got[p]++; else ++pads;
    }
    CHECK(want == got && pads == order.size() - (size_t)cnt);
    // in a batch: ascending rank, pads only behind the rows; batches: costs
    // finite, positive and non-increasing, equal costs in rank order
    int padded = 0;
    for (int32_t b = 0; b < nB; ++b) {
        int c = 0;
        for (int l = 0; l < LB; ++l) {
            const int32_t p = order[(size_t)b * LB + l];
            if (p < 0) continue;
            CHECK(c == l);
            if (l > 0 && c == l) CHECK(br.rank[order[(size_t)b * LB + l - 1]] < br.rank[p]);
            ++c;
        }
        CHECK(c > 0);
        padded += c < LB;
        CHECK(std::isfinite(cost[b]) && cost[b] > 0.0);
        if (b > 0) CHECK(cost[b - 1] >= cost[b]);
        if (b > 0 && cost[b - 1] == cost[b]) CHECK(br.rank[order[(size_t)(b - 1) * LB]] < br.rank[order[(size_t)b * LB]]);
    }
    CHECK(padded == (cnt % LB != 0));
    // the same batches as batch_order's, whatever their sequence
    std::vector<int32_t> plain = batch_order(br.rank, br.rowOff, LB, pos.data(), cnt, nB1);
    CHECK(nB1 == nB && plain.size() == order.size());
    if (plain.size() != order.size()) return;
    std::vector<std::vector<int32_t>> a, b;
    for (int32_t i = 0; i < nB; ++i) {
        a.emplace_back(order.begin() + (size_t)i * LB, order.begin() + (size_t)(i + 1) * LB);
        b.emplace_back(plain.begin() + (size_t)i * LB, plain.begin() + (size_t)(i + 1) * LB);
    }
    std::sort(a.begin(), a.end());
    std::sort(b.begin(), b.end());
    CHECK(a == b);
    // the key is scale-free: latencies and unit times 4 give the same costs
    BatchRanks x4 = br;
    for (double& d : x4.rowOff) d *= 4.0;
    for (double& d : x4.groups.dist) d *= 4.0;
    std::vector<double> cost4;
    const std::vector<int32_t> order4 =
        batch_order_cost(x4.rank, x4.rowOff, x4.groups, unit * 4.0, LB, pos.data(), cnt, nB1, &cost4);
    CHECK(order4 == order && same_bytes(cost4, cost));
}

void test_case(const Case& c) {
    const HostGraph& g = c.g;
    const int32_t T = (int32_t)c.attached.size();
    const int32_t K = (int32_t)std::max<int64_t>(1, std::min<int64_t>(256, g.n / 400));
    CHECK(T % 8 != 0);
    const HubGroups hg = test_groups(c, K);
    const BatchRanks br = batch_ranks(g, c.attached, c.posOf, 2);
    const BatchRanks br1 = batch_ranks(g, c.attached, c.posOf, 1);
    CHECK(br1.groups.empty() && br.groups.G == hg.G);
    CHECK(same_bytes(br.groups.dist, hg.dist) && same_bytes(br.groups.hub, hg.hub));
    CHECK((int32_t)br.rank.size() == T && (int32_t)br.rowOff.size() == T);
    if ((int32_t)br.rank.size() != T || (int32_t)br.rowOff.size() != T || hg.dist.size() != (size_t)T * hg.G) return;
    // ranks: a permutation, ascending in the key; no hub: last, offset 0
    std::vector<int32_t> at(T, -1);
    for (int32_t p = 0; p < T; ++p) {
        CHECK(br.rank[p] >= 0 && br.rank[p] < T && at[br.rank[p]] < 0);
        if (br.rank[p] >= 0 && br.rank[p] < T) at[br.rank[p]] = p;
    }
    bool lost = false;
    for (int32_t r = 0; r < T; ++r) {
        if (at[r] < 0) return;
        const Key k = key_of(hg, at[r]);
        if (r > 0) CHECK(key_less(key_of(hg, at[r - 1]), k));
        if (k.h1 == INT32_MAX) lost = true;
        CHECK(lost == (k.h1 == INT32_MAX));
        // the offset: the minimum over the groups, which is order 1's
        // distance to the nearest hub
        double mn = INFINITY;
        for (int j = 0; j < hg.G; ++j) mn = std::min(mn, hg.dist[(size_t)at[r] * hg.G + j]);
        CHECK(same_bits(br.rowOff[at[r]], std::isfinite(mn) ? mn : 0.0));
        CHECK(same_bits(br.rowOff[at[r]], br1.rowOff[at[r]]));
    }
    // all positions (T no multiple of LB), a subset, and a single batch
    std::vector<int32_t> all(T), third, few;
    for (int32_t p = 0; p < T; ++p) all[p] = T - 1 - p;
    for (int32_t p = 0; p < T; p += 3) third.push_back(p);
    for (int32_t p = 0; p < std::min(T, 5); ++p) few.push_back((p * 7) % T);
    std::sort(few.begin(), few.end());
    few.erase(std::unique(few.begin(), few.end()), few.end());
    for (int LB : {8, 16}) {
        check_cost_order(br, g.meanArcLatency, LB, all);
        check_cost_order(br, g.meanArcLatency, LB, third);
        check_cost_order(br, g.meanArcLatency, LB, few);
    }
}

// Spread and offset both raise the cost; a padded batch costs its share.
void test_cost_terms() {
    BatchRanks br;
    const int T = 20, G = HUB_GROUPS;
    br.rank.resize(T);
    br.rowOff.assign(T, 1.0);
    br.groups.G = G;
    br.groups.dist.assign((size_t)T * G, INFINITY);
    br.groups.hub.assign((size_t)T * G, INT32_MAX);
    for (int p = 0; p < T; ++p) {
        br.rank[p] = p;
        br.groups.dist[(size_t)p * G] = 1.0;                                 // its own hub
        br.groups.dist[(size_t)p * G + 1] = p < 4 ? 5.0 : p < 8 ? 5.0 + p : 3.0;   // batch 1 is out of step
    }
    for (int p = 8; p < 12; ++p) br.rowOff[p] = br.groups.dist[(size_t)p * G] = 2.0;   // batch 2 is further out
    for (int p = 8; p < 12; ++p) br.groups.dist[(size_t)p * G + 1] = 4.0;
    std::vector<int32_t> pos(T - 2);
    for (int p = 0; p < T - 2; ++p) pos[p] = p;
    int32_t nB = 0;
    std::vector<double> cost;
    const std::vector<int32_t> order = batch_order_cost(br.rank, br.rowOff, br.groups, 1.0, 4, pos.data(), T - 2, nB, &cost);
    // batches of positions 0-3 (even), 4-7 (spread), 8-11 (offset), 12-15 (even), 16-17 (padded)
    CHECK(nB == 5 && order.size() == 20);
    if (order.size() != 20) return;
    CHECK(order[0] == 4 && order[4] == 8 && order[8] == 0 && order[12] == 12 && order[16] == 16 && order[18] == -1);
    CHECK(cost[0] > cost[1] && cost[1] > cost[2] && cost[2] == cost[3] && same_bits(cost[4], cost[3] * 0.5));
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: plan_cost DIR...\n"); return 2; }
    for (int i = 1; i < argc; ++i) {
        const Case c = load(argv[i]);
        test_case(c);
        std::printf("%s: n %d arcs %lld directed %d attached %zu\n", argv[i], c.g.n, (long long)c.g.nArcs(),
                    c.g.directed, c.attached.size());
    }
    test_cost_terms();
    if (failures) return 1;
    std::printf("OK\n");
    return 0;
}
