// batch_order_cost of pe_plan.cpp as a record: per graph directory (the layout
// of tests/native/plan_cost.cpp), lane count, offset kind and position set one
// line with a 64-bit FNV-1a hash each of the batch rows, the costs' bit patterns
// and the lane offsets' bit patterns.  tests/test_plan_order_cost.py compares the
// lines with tests/golden/plan_order_cost.txt, recorded before the plan moved to
// the device: the host planner, the reference of the device plan, computes what
// it computed.  Built with pe_plan.cpp and pe_graph.cpp; no HIP.
//
//   plan_order_cost NAME=DIR...
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "pe_graph.hpp"
#include "pe_plan.hpp"

using namespace shdpe;

namespace {

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

template <class T>
unsigned long long fnv(const std::vector<T>& v) {
    unsigned long long h = 1469598103934665603ull;
    const unsigned char* p = reinterpret_cast<const unsigned char*>(v.data());
    for (size_t i = 0; i < v.size() * sizeof(T); ++i) h = (h ^ p[i]) * 1099511628211ull;
    return h;
}

void record(const std::string& name, const std::string& dir) {
    int n = 0, directed = 0, hasVloss = 0;
    FILE* f = std::fopen((dir + "/meta.txt").c_str(), "r");
    if (!f || std::fscanf(f, "%d %d %d", &n, &directed, &hasVloss) != 3) std::exit(2);
    std::fclose(f);
    const auto from = read_array<int32_t>(dir + "/from.i32"), to = read_array<int32_t>(dir + "/to.i32");
    const auto lat = read_array<double>(dir + "/lat.f64"), loss = read_array<double>(dir + "/loss.f64");
    const auto vloss = hasVloss ? read_array<double>(dir + "/vloss.f64") : std::vector<double>();
    ShdPeGraphDesc d{n, (int64_t)from.size(), directed, from.data(), to.data(), lat.data(), loss.data(),
                     hasVloss ? vloss.data() : nullptr};
    HostGraph g;
    if (build_host_graph(&d, &g) != SHD_PE_OK) std::exit(2);
    std::vector<int32_t> attached, posOf(g.n, -1);
    for (int32_t v : read_array<int32_t>(dir + "/att.i32"))
        if (posOf[v] < 0) { posOf[v] = (int32_t)attached.size(); attached.push_back(v); }
    const int32_t T = (int32_t)attached.size();
    const BatchRanks br = batch_ranks(g, attached, posOf, 2);
    // all positions from the last to the first, every third, and one short batch
    std::vector<std::vector<int32_t>> sets(3);
    for (int32_t p = 0; p < T; ++p) sets[0].push_back(T - 1 - p);
    for (int32_t p = 0; p < T; p += 3) sets[1].push_back(p);
    for (int32_t p = 0; p < 5 && p < T; ++p) sets[2].push_back(T - 1 - 2 * p);
    for (int LB : {8, 16})
        for (int kind : {0, 1})
            for (size_t s = 0; s < sets.size(); ++s) {
                int32_t nB = 0;
                std::vector<double> cost, off;
                const std::vector<int32_t> order =
                    batch_order_cost(br.rank, br.rowOff, br.groups, g.meanArcLatency, LB, sets[s].data(),
                                     (int32_t)sets[s].size(), nB, &cost, &off, kind);
                std::printf("%s lb %d kind %d set %zu batches %d rows %016llx costs %016llx offsets %016llx\n",
                            name.c_str(), LB, kind, s, nB, fnv(order), fnv(cost), fnv(off));
            }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: plan_order_cost NAME=DIR...\n"); return 2; }
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        const size_t eq = a.find('=');
        if (eq == std::string::npos) return 2;
        record(a.substr(0, eq), a.substr(eq + 1));
    }
    return 0;
}
