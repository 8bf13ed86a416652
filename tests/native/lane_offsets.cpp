// lane_offsets of pe_plan.cpp (the per-(batch, lane) bucket key offsets) and
// batch_order_cost's use of them, over graphs that tests/test_lane_offsets.py
// writes as raw arrays in the layout of tests/native/plan_cost.cpp's graph
// directories, and over synthetic hub-group distances.  Built with
// pe_plan.cpp and pe_graph.cpp, -fsanitize=address,undefined; no HIP.
//
//   lane_offsets DIR...    every check on every graph, "OK" when all hold
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
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
bool is_zero(double a) { return same_bits(a, 0.0); }

struct Tally { int batches = 0, leastSquares = 0, fallback = 0, oneLane = 0, padded = 0; };

// What every result of lane_offsets must satisfy, batch by batch, and what
// kind 1 must give against sums of its own (the formula of pe_plan.hpp with
// its means: equal to the result within rounding).
void check_offsets(const HubGroups& hg, const std::vector<double>& rowOff, const std::vector<int32_t>& order,
                   int LB, const std::vector<double>& off, double unit, Tally* tally) {
    CHECK(off.size() == order.size() && order.size() % LB == 0);
    if (off.size() != order.size()) return;
    const int G = hg.G;
    for (size_t b0 = 0; b0 < order.size(); b0 += LB) {
        std::vector<int> real;
        for (int l = 0; l < LB; ++l) {
            if (order[b0 + l] >= 0) real.push_back(l);
            else CHECK(is_zero(off[b0 + l]));                       // pads are 0
            CHECK(std::isfinite(off[b0 + l]) && off[b0 + l] >= 0.0);
        }
        std::vector<int> J;
        for (int j = 0; j < G; ++j) {
            bool all = !real.empty();
            for (int l : real) all = all && std::isfinite(hg.dist[(size_t)order[b0 + l] * G + j]);
            if (all) J.push_back(j);
        }
        if (tally) { ++tally->batches; tally->padded += (int)real.size() < LB; }
        if (J.empty()) {          // a lane no hub reaches (or no groups): exactly the nearest-hub distance
            for (int l : real) CHECK(same_bits(off[b0 + l], rowOff.empty() ? 0.0 : rowOff[order[b0 + l]]));
            if (tally) ++tally->fallback;
            continue;
        }
        if (tally) { ++tally->leastSquares; tally->oneLane += real.size() == 1; }
        double mn = INFINITY;
        for (int l : real) mn = std::min(mn, off[b0 + l]);
        CHECK(is_zero(mn));                                         // the batch minimum is exactly 0
        if (real.size() == 1) CHECK(is_zero(off[b0 + real[0]]));
        // s_l = mean over J of (d[l][j] - mean over the lanes of d[.][j]), less its minimum
        std::vector<double> s(LB, 0.0);
        for (int j : J) {
            double mean = 0.0;
            for (int l : real) mean += hg.dist[(size_t)order[b0 + l] * G + j];
            mean /= (double)real.size();
            for (int l : real) s[l] += (hg.dist[(size_t)order[b0 + l] * G + j] - mean) / (double)J.size();
        }
        double smin = INFINITY;
        for (int l : real) smin = std::min(smin, s[l]);
        for (int l : real) CHECK(std::fabs(off[b0 + l] - (s[l] - smin)) <= 1e-9 * unit);
    }
}

// The lanes of every batch reversed and rotated: the offsets move with them.
void check_lane_permutation(const HubGroups& hg, const std::vector<double>& rowOff,
                            const std::vector<int32_t>& order, int LB, const std::vector<double>& off) {
    std::vector<int32_t> perm(order.size());
    std::vector<int> from(order.size());
    for (size_t b0 = 0; b0 < order.size(); b0 += LB)
        for (int l = 0; l < LB; ++l) {
            const int src = (LB - 1 - l + 3) % LB;
            perm[b0 + l] = order[b0 + src];
            from[b0 + l] = (int)b0 + src;
        }
    const std::vector<double> o = lane_offsets(hg, rowOff, perm, LB, 1);
    CHECK(o.size() == off.size());
    if (o.size() != off.size()) return;
    for (size_t i = 0; i < o.size(); ++i) CHECK(same_bits(o[i], off[(size_t)from[i]]));
}

void check_batch_order_cost(const BatchRanks& br, double unit, int LB, const std::vector<int32_t>& pos,
                            Tally* tally) {
    const int32_t T = (int32_t)br.rank.size(), cnt = (int32_t)pos.size();
    for (int kind : {1, 0}) {
        int32_t nB = -1, nB1 = -1;
        std::vector<double> cost, off;
        const std::vector<int32_t> order =
            batch_order_cost(br.rank, br.rowOff, br.groups, unit, LB, pos.data(), cnt, nB, &cost, &off, kind);
        CHECK(nB == (cnt + LB - 1) / LB && order.size() == (size_t)nB * LB && cost.size() == (size_t)nB);
        CHECK(off.size() == order.size());
        if (order.size() != (size_t)nB * LB || cost.size() != (size_t)nB || off.size() != order.size()) return;
        // every position once, pads last in their batch, costs non-increasing
        std::vector<int> want(T, 0), got(T, 0);
        for (int32_t p : pos) want[p]++;
        size_t pads = 0;
        for (int32_t p : order) {
            CHECK(p >= -1 && p < T);
            if (p >= 0 && p < T) got[p]++; else ++pads;
        }
        CHECK(want == got && pads == order.size() - (size_t)cnt);
        for (int32_t b = 0; b < nB; ++b) {
            bool pad = false;
            for (int l = 0; l < LB; ++l) {
                if (order[(size_t)b * LB + l] < 0) pad = true;
                else CHECK(!pad);
            }
            CHECK(order[(size_t)b * LB] >= 0);
            CHECK(std::isfinite(cost[b]) && cost[b] > 0.0);
            if (b > 0) CHECK(cost[b - 1] >= cost[b]);
        }
        // the offsets belong to the batches in their final sequence
        CHECK(same_bytes(off, lane_offsets(br.groups, br.rowOff, order, LB, kind)));
        if (kind == 0)
            for (size_t i = 0; i < order.size(); ++i)
                CHECK(same_bits(off[i], order[i] >= 0 ? br.rowOff[order[i]] : 0.0));
        check_offsets(br.groups, br.rowOff, order, LB, kind == 1 ? off : lane_offsets(br.groups, br.rowOff, order, LB, 1),
                      unit, kind == 1 ? tally : nullptr);
        if (kind == 1) check_lane_permutation(br.groups, br.rowOff, order, LB, off);
        // the same batches as batch_order's, whatever their sequence and the offsets
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
        // batch_order's batches (the path tier's): the same rules
        check_offsets(br.groups, br.rowOff, plain, LB, lane_offsets(br.groups, br.rowOff, plain, LB, 1), unit, nullptr);
    }
}

Tally test_case(const Case& c) {
    Tally tally;
    const HostGraph& g = c.g;
    const int32_t T = (int32_t)c.attached.size();
    CHECK(T % 8 != 0);
    // the plan on 1 and on 16 planner threads: the same offsets
    const BatchRanks br = batch_ranks(g, c.attached, c.posOf, 2);
    BatchRanks one, many;
    one.groups = hub_group_distances(g, c.attached, 1);
    many.groups = hub_group_distances(g, c.attached, 16);
    CHECK(same_bytes(one.groups.dist, br.groups.dist) && same_bytes(many.groups.dist, br.groups.dist));
    std::vector<int32_t> all(T), third, few, single;
    for (int32_t p = 0; p < T; ++p) all[p] = T - 1 - p;
    for (int32_t p = 0; p < T; p += 3) third.push_back(p);
    for (int32_t p = 0; p < std::min(T, 5); ++p) few.push_back((p * 7) % T);
    std::sort(few.begin(), few.end());
    few.erase(std::unique(few.begin(), few.end()), few.end());
    single.push_back(T / 2);
    for (int LB : {8, 16}) {
        int32_t nB = 0;
        std::vector<double> o1, o16, ob;
        const std::vector<int32_t> order =
            batch_order_cost(br.rank, br.rowOff, br.groups, g.meanArcLatency, LB, all.data(), T, nB, nullptr, &ob);
        const std::vector<int32_t> order1 =
            batch_order_cost(br.rank, br.rowOff, one.groups, g.meanArcLatency, LB, all.data(), T, nB, nullptr, &o1);
        const std::vector<int32_t> order16 =
            batch_order_cost(br.rank, br.rowOff, many.groups, g.meanArcLatency, LB, all.data(), T, nB, nullptr, &o16);
        CHECK(order == order1 && order == order16 && same_bytes(ob, o1) && same_bytes(ob, o16));
        check_batch_order_cost(br, g.meanArcLatency, LB, all, &tally);
        check_batch_order_cost(br, g.meanArcLatency, LB, third, &tally);
        check_batch_order_cost(br, g.meanArcLatency, LB, few, &tally);
        check_batch_order_cost(br, g.meanArcLatency, LB, single, &tally);
        // orders 0 and 1 have no groups: the nearest-hub distance, or 0
        for (int ord : {0, 1}) {
            const BatchRanks b01 = batch_ranks(g, c.attached, c.posOf, ord);
            CHECK(b01.groups.empty());
            const std::vector<int32_t> o = batch_order(b01.rank, b01.rowOff, LB, all.data(), T, nB);
            for (int kind : {0, 1}) {
                const std::vector<double> off = lane_offsets(b01.groups, b01.rowOff, o, LB, kind);
                CHECK(off.size() == o.size());
                for (size_t i = 0; i < off.size() && i < o.size(); ++i)
                    CHECK(same_bits(off[i], o[i] >= 0 && ord == 1 ? b01.rowOff[o[i]] : 0.0));
            }
        }
    }
    return tally;
}

// d[l][j] = c_j + t_l in dyadic values: the offsets are t_l - min t exactly,
// whatever constant is added to every distance and whichever groups are
// empty; a lane with an infinite group takes that group out; a lane that no
// group reaches sends its batch back to rowOff.
void test_synthetic() {
    const int G = HUB_GROUPS, T = 37;
    for (int LB : {8, 16}) {
        for (int used : {1, 3, 16}) {           // groups `used`.. are empty, as with K < 16 hubs
            HubGroups hg;
            hg.G = G;
            hg.dist.assign((size_t)T * G, INFINITY);
            hg.hub.assign((size_t)T * G, INT32_MAX);
            std::vector<double> t(T), rowOff(T);
            for (int p = 0; p < T; ++p) {
                t[p] = ((p * 29) % 64) / 64.0 + (p % 3) * 0.5;
                for (int j = 0; j < used; ++j) hg.dist[(size_t)p * G + j] = 2.0 + j * 0.375 + t[p];
                rowOff[p] = 2.0 + t[p];
            }
            std::vector<int32_t> order;
            for (int p = 0; p < T; ++p) order.push_back((p * 5) % T);
            order.resize((size_t)(T + LB - 1) / LB * LB, -1);
            const std::vector<double> off = lane_offsets(hg, rowOff, order, LB, 1);
            CHECK(off.size() == order.size());
            if (off.size() != order.size()) return;
            for (size_t b0 = 0; b0 < order.size(); b0 += LB) {
                double tmin = INFINITY;
                for (int l = 0; l < LB; ++l)
                    if (order[b0 + l] >= 0) tmin = std::min(tmin, t[order[b0 + l]]);
                for (int l = 0; l < LB; ++l)
                    CHECK(same_bits(off[b0 + l], order[b0 + l] >= 0 ? t[order[b0 + l]] - tmin : 0.0));
            }
            check_offsets(hg, rowOff, order, LB, off, 1.0, nullptr);
            check_lane_permutation(hg, rowOff, order, LB, off);
            // one constant on every lane's distances: nothing changes
            HubGroups up = hg;
            for (double& d : up.dist) d += 1024.0;
            CHECK(same_bytes(lane_offsets(up, rowOff, order, LB, 1), off));
            // a group that is infinite for all lanes where it was finite: as if it never was
            if (used > 1) {
                HubGroups fewer = hg;
                for (int p = 0; p < T; ++p) fewer.dist[(size_t)p * G + used - 1] = INFINITY;
                CHECK(same_bytes(lane_offsets(fewer, rowOff, order, LB, 1), off));
                // ... infinite for one lane only: its batch does without the group, the others keep it
                HubGroups hole = hg;
                hole.dist[(size_t)order[1] * G + used - 1] = INFINITY;
                CHECK(same_bytes(lane_offsets(hole, rowOff, order, LB, 1), off));
            }
            // a lane no group reaches: its batch gets rowOff, bit for bit; the others are untouched
            HubGroups lost = hg;
            for (int j = 0; j < G; ++j) lost.dist[(size_t)order[LB + 2] * G + j] = INFINITY;
            const std::vector<double> offLost = lane_offsets(lost, rowOff, order, LB, 1);
            for (size_t i = 0; i < order.size(); ++i) {
                const bool second = i >= (size_t)LB && i < (size_t)2 * LB;
                CHECK(same_bits(offLost[i], second ? (order[i] >= 0 ? rowOff[order[i]] : 0.0) : off[i]));
            }
            // kind 0: rowOff everywhere
            const std::vector<double> off0 = lane_offsets(hg, rowOff, order, LB, 0);
            for (size_t i = 0; i < order.size(); ++i)
                CHECK(same_bits(off0[i], order[i] >= 0 ? rowOff[order[i]] : 0.0));
        }
    }
    // no positions at all
    CHECK(lane_offsets(HubGroups(), std::vector<double>(), std::vector<int32_t>(), 16, 1).empty());
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: lane_offsets DIR...\n"); return 2; }
    for (int i = 1; i < argc; ++i) {
        const Case c = load(argv[i]);
        const Tally t = test_case(c);
        std::printf("%s: n %d directed %d attached %zu batches %d least-squares %d fallback %d one-lane %d padded %d\n",
                    argv[i], c.g.n, c.g.directed, c.attached.size(), t.batches, t.leastSquares, t.fallback,
                    t.oneLane, t.padded);
    }
    test_synthetic();
    if (failures) return 1;
    std::printf("OK\n");
    return 0;
}
