// Stand-alone driver of shd_pe_graph_props_host (pe_props.cpp), built with
// -fsanitize=address,undefined by tests/test_props.py and linked with
// pe_props.cpp only.
//
//   props <dump>
//
// <dump> is a text file of cases, each
//   case <name> <n> <directed> <m> <clusterCount> <largestCluster> <isComplete> <firstIncomplete>
//   m lines "<from> <to>"
//   n membership values
// Every case is run with and without a membership array and compared with
// the expected values.  Then a 250,000-vertex directed chain (n clusters:
// the recursion-depth check), the same chain closed into a ring (1 cluster)
// and the argument errors.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "shd_pathengine.h"

static int fails = 0;
#define CHECK(c, ...)                                  \
    do {                                               \
        if (!(c)) {                                    \
            ++fails;                                   \
            std::fprintf(stderr, "FAIL %s: ", #c);     \
            std::fprintf(stderr, __VA_ARGS__);         \
            std::fprintf(stderr, "\n");                \
        }                                              \
    } while (0)

static ShdPeGraphDesc desc(int32_t n, bool directed, const std::vector<int32_t>& f, const std::vector<int32_t>& t) {
    ShdPeGraphDesc g;
    std::memset(&g, 0, sizeof(g));                 // latency / loss pointers stay NULL
    g.nVertices = n;
    g.nEdges = (int64_t)f.size();
    g.directed = directed;
    g.edgeFrom = f.data();
    g.edgeTo = t.data();
    return g;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: props <dump>\n");
        return 2;
    }
    std::FILE* fp = std::fopen(argv[1], "r");
    if (!fp) {
        std::perror(argv[1]);
        return 2;
    }
    int nCases = 0;
    char name[128];
    int n, directed, clusters, largest, complete, first;
    long long m;
    while (std::fscanf(fp, " case %127s %d %d %lld %d %d %d %d", name, &n, &directed, &m, &clusters, &largest,
                       &complete, &first) == 8) {
        std::vector<int32_t> f((size_t)m), t((size_t)m), want((size_t)n), got((size_t)n, -7);
        for (long long e = 0; e < m; ++e)
            if (std::fscanf(fp, "%d %d", &f[(size_t)e], &t[(size_t)e]) != 2) return 2;
        for (int v = 0; v < n; ++v)
            if (std::fscanf(fp, "%d", &want[(size_t)v]) != 1) return 2;
        const ShdPeGraphDesc g = desc(n, directed != 0, f, t);
        for (int withMem = 0; withMem < 2; ++withMem) {
            ShdPeGraphProps p;
            std::memset(&p, 0xff, sizeof(p));
            const int rc = shd_pe_graph_props_host(&g, &p, withMem ? got.data() : nullptr);
            CHECK(rc == 0, "%s rc %d", name, rc);
            CHECK(p.isDirected == (directed != 0), "%s", name);
            CHECK(p.clusterCount == clusters, "%s clusters %d want %d", name, p.clusterCount, clusters);
            CHECK(p.isConnected == (clusters == 1), "%s", name);
            CHECK(p.largestCluster == largest, "%s largest %d want %d", name, p.largestCluster, largest);
            CHECK(p.isComplete == complete, "%s complete %d", name, p.isComplete);
            CHECK(p.firstIncomplete == first, "%s first %d want %d", name, p.firstIncomplete, first);
        }
        CHECK(got == want, "%s membership", name);
        ++nCases;
    }
    std::fclose(fp);
    CHECK(nCases > 0, "no case in %s", argv[1]);

    {   // recursion depth: a recursive SCC overflows the stack here
        const int32_t N = 250000;
        std::vector<int32_t> f((size_t)N - 1), t((size_t)N - 1), mem((size_t)N);
        for (int32_t v = 0; v + 1 < N; ++v) { f[(size_t)v] = v; t[(size_t)v] = v + 1; }
        ShdPeGraphProps p;
        ShdPeGraphDesc g = desc(N, true, f, t);
        CHECK(shd_pe_graph_props_host(&g, &p, mem.data()) == 0, "chain");
        CHECK(p.clusterCount == N && p.largestCluster == 1 && !p.isConnected, "chain clusters %d", p.clusterCount);
        bool own = true;
        for (int32_t v = 0; v < N; ++v) own = own && mem[(size_t)v] == v;
        CHECK(own, "chain membership");
        f.push_back(N - 1);
        t.push_back(0);
        g = desc(N, true, f, t);
        CHECK(shd_pe_graph_props_host(&g, &p, mem.data()) == 0, "ring");
        CHECK(p.clusterCount == 1 && p.largestCluster == N && p.isConnected, "ring clusters %d", p.clusterCount);
        g.directed = 0;                            // the undirected path of the same length
        g.nEdges = N - 1;
        CHECK(shd_pe_graph_props_host(&g, &p, mem.data()) == 0, "path");
        CHECK(p.clusterCount == 1 && mem[(size_t)N - 1] == 0, "path clusters %d", p.clusterCount);
    }
    {   // argument errors
        std::vector<int32_t> f{0, 1}, t{1, 2};
        ShdPeGraphProps p;
        ShdPeGraphDesc g = desc(2, true, f, t);    // endpoint == n
        CHECK(shd_pe_graph_props_host(&g, &p, nullptr) == SHD_PE_EINVAL, "endpoint n");
        t[1] = -1;
        CHECK(shd_pe_graph_props_host(&g, &p, nullptr) == SHD_PE_EINVAL, "endpoint -1");
        t[1] = 0;
        CHECK(shd_pe_graph_props_host(&g, &p, nullptr) == 0, "valid");
        CHECK(shd_pe_graph_props_host(&g, nullptr, nullptr) == SHD_PE_EINVAL, "NULL out");
        g.nVertices = 0;
        CHECK(shd_pe_graph_props_host(&g, &p, nullptr) == SHD_PE_EINVAL, "n = 0");
        g.nVertices = 2;
        g.nEdges = (int64_t)INT32_MAX / 2 + 1;     // refused before any edge is read
        CHECK(shd_pe_graph_props_host(&g, &p, nullptr) == SHD_PE_ETOOBIG, "too big");
    }
    if (fails) return 1;
    std::printf("OK %d cases\n", nCases);
    return 0;
}
