// pe_props.cpp -- graph property check on the host (no HIP).
//
//   shd_pe_graph_props_host   _topology_checkGraphProperties   topology.c:724-809
//     isConnected / clusterCount   igraph_is_connected / igraph_clusters (STRONG)  :738, :745
//     isComplete / firstIncomplete _topology_isComplete                            :450-552
//
// The late or CPU-only path, the device form's hand-off target (pe_props.hip)
// and the tests' second opinion.  One counting pass for completeness (the rule
// pe_graph.cpp states for the engine); clusters by union-find (undirected: weak
// components) or an iterative Tarjan over a CSR built here (directed: strong
// components; an explicit stack, since recursion overflows on a 250k chain).
#include <algorithm>
#include <cstdint>
#include <new>
#include <vector>

#include "shd_pathengine.h"

namespace {

// membership[v] = smallest id of v's weak component
void weak_components(int32_t n, int64_t m, const int32_t* from, const int32_t* to, int32_t* mem) {
    for (int32_t v = 0; v < n; ++v) mem[v] = v;
    auto find = [&](int32_t x) {
        while (mem[x] != x) {
            mem[x] = mem[mem[x]];       // path halving
            x = mem[x];
        }
        return x;
    };
    for (int64_t e = 0; e < m; ++e) {
        const int32_t a = find(from[e]), b = find(to[e]);
        if (a < b) mem[b] = a;          // the root is the smaller id: parents only decrease
        else if (b < a) mem[a] = b;
    }
    for (int32_t v = 0; v < n; ++v) mem[v] = find(v);
}

// membership[v] = smallest id of v's strong component (Tarjan, explicit stack)
void strong_components(int32_t n, int64_t m, const int32_t* from, const int32_t* to, int32_t* mem) {
    std::vector<int64_t> ptr((size_t)n + 1, 0);
    for (int64_t e = 0; e < m; ++e) ptr[(size_t)from[e] + 1]++;
    for (int32_t v = 0; v < n; ++v) ptr[(size_t)v + 1] += ptr[v];
    std::vector<int32_t> col((size_t)m);
    {
        std::vector<int64_t> fill(ptr.begin(), ptr.end() - 1);
        for (int64_t e = 0; e < m; ++e) col[(size_t)fill[from[e]]++] = to[e];
    }
    std::vector<int32_t> index((size_t)n, -1), low((size_t)n, 0), stack, calls;
    std::vector<int64_t> it(ptr.begin(), ptr.end() - 1);      // next arc of each vertex
    std::vector<uint8_t> onStack((size_t)n, 0);
    int32_t next = 0;
    for (int32_t r = 0; r < n; ++r) {
        if (index[r] >= 0) continue;
        index[r] = low[r] = next++;
        stack.push_back(r);
        onStack[r] = 1;
        calls.push_back(r);
        while (!calls.empty()) {
            const int32_t v = calls.back();
            if (it[v] < ptr[(size_t)v + 1]) {
                const int32_t w = col[(size_t)it[v]++];
                if (index[w] < 0) {
                    index[w] = low[w] = next++;
                    stack.push_back(w);
                    onStack[w] = 1;
                    calls.push_back(w);
                } else if (onStack[w]) {
                    low[v] = std::min(low[v], index[w]);
                }
                continue;
            }
            calls.pop_back();
            if (!calls.empty()) low[calls.back()] = std::min(low[calls.back()], low[v]);
            if (low[v] != index[v]) continue;
            // v is a root: its component is the stack down to v
            size_t k = stack.size();
            int32_t mn = v;
            do { --k; mn = std::min(mn, stack[k]); } while (stack[k] != v);
            for (size_t j = k; j < stack.size(); ++j) {
                mem[stack[j]] = mn;
                onStack[stack[j]] = 0;
            }
            stack.resize(k);
        }
    }
}

}  // namespace

extern "C" int shd_pe_graph_props_host(const ShdPeGraphDesc* g, ShdPeGraphProps* out, int32_t* membership) {
    if (!g || !out || g->nVertices <= 0 || g->nEdges < 0) return SHD_PE_EINVAL;
    if (g->nEdges > 0 && (!g->edgeFrom || !g->edgeTo)) return SHD_PE_EINVAL;
    if (g->nEdges > INT32_MAX / 2) return SHD_PE_ETOOBIG;
    const int32_t n = g->nVertices;
    const int64_t m = g->nEdges;
    const int32_t *from = g->edgeFrom, *to = g->edgeTo;
    const bool directed = g->directed != 0;
    try {
        // _topology_isComplete: OUT-incident edges per vertex, parallel edges each
        std::vector<int32_t> cnt((size_t)n, 0);
        std::vector<uint8_t> hasSelf((size_t)n, 0);
        for (int64_t e = 0; e < m; ++e) {
            const int32_t f = from[e], t = to[e];
            if (f < 0 || f >= n || t < 0 || t >= n) return SHD_PE_EINVAL;
            cnt[f]++;
            if (!directed) {
                cnt[t]++;                                  // a self-loop counts twice ...
                if (f == t) hasSelf[f] = 1;
            }
        }
        int32_t firstIncomplete = -1;
        for (int32_t v = 0; v < n; ++v)
            if (cnt[v] - (int32_t)hasSelf[v] < n) { firstIncomplete = v; break; }   // ... minus one, once
        std::vector<int32_t> own;
        int32_t* mem = membership;
        if (!mem) {
            own.resize((size_t)n);
            mem = own.data();
        }
        if (directed) strong_components(n, m, from, to, mem);
        else weak_components(n, m, from, to, mem);
        // cluster sizes in the counting array (done with it)
        std::fill(cnt.begin(), cnt.end(), 0);
        int32_t clusters = 0, largest = 0;
        for (int32_t v = 0; v < n; ++v) {
            clusters += mem[v] == v;
            largest = std::max(largest, ++cnt[mem[v]]);
        }
        out->isDirected = directed;
        out->isConnected = clusters == 1;
        out->clusterCount = clusters;
        out->largestCluster = largest;
        out->isComplete = firstIncomplete < 0;
        out->firstIncomplete = firstIncomplete;
    } catch (const std::bad_alloc&) {
        return SHD_PE_ENOMEM;
    }
    return SHD_PE_OK;
}
