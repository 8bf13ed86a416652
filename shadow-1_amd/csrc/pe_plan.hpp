// pe_plan.hpp -- what shd_pe_create decides on the host before anything is
// uploaded: the device vertex ids (degree relabelling), the batch schedule
// (ranks, hub offsets, batch order), the compute mode and the row-shard plan.
// Free functions over HostGraph and plain vectors: no GPU types, no engine
// state, so tests/native/plan.cpp drives them on the CPU under sanitizers.
#pragma once
#include <stdint.h>

#include <vector>

#include "pe_graph.hpp"

namespace shdpe {

// The vertices by descending out-degree, equal degrees in ascending id
// (stable): the device ids of the batched path (relabel_graph) and, its first
// K entries, the hubs of batch order 1.
std::vector<int32_t> degree_order(const HostGraph& g);

// The graph with vertex k = g's vertex oldOf[k] (oldOf a permutation of
// 0..n-1): per-vertex arrays permuted, arc targets renamed, outToIn rebuilt,
// scalars copied.  Every row keeps its arcs in the sequence of g's row --
// igraph incidence order by the CALLER's ids -- so every pop / push order of
// the kernels, and the tie-breaking that depends on it, is that of g.
// findArc is INVALID on the result (rows are not ascending in the new ids):
// it is for upload only, lookups stay on g.
HostGraph relabel_graph(const HostGraph& g, const std::vector<int32_t>& oldOf);

// Batch order of the table positions: sources of one batch should have
// similar distance profiles so their delta-stepping frontiers coincide.
//   order 0: BFS visit rank (components in vertex order); rowOff stays empty;
//   order 1 (default): nearest-hub cells -- a multi-source Dijkstra from
//            the K highest-degree vertices gives every vertex its closest
//            hub; sources sort by (hub, distance to it), so a batch holds
//            sources that reach the rest of the graph through one hub, and
//            the distance to the hub becomes the lane's bucket key offset
//            (k_batch_rows: a lane's key is dist + maxOff - off).
// Scheduling only: results never depend on it (tools/sim/ models the
// schedule: C4 arc visits 3.9 -> 2.2 x m per batch with offsets, dirty
// lanes and a far set at delta = mean arc latency).
struct BatchRanks {
    std::vector<int32_t> rank;     // table position -> batch order rank
    std::vector<double> rowOff;    // table position -> distance to its batch hub (order 1)
};
BatchRanks batch_ranks(const HostGraph& g, const std::vector<int32_t>& attached,
                       const std::vector<int32_t>& posOf, int order);

// Batches of LB nearby sources (rank order) out of the cnt positions pos[],
// -1 pads the last; nB = their number.  With rowOff, longest batches first.
std::vector<int32_t> batch_order(const std::vector<int32_t>& rank, const std::vector<double>& rowOff,
                                 int LB, const int32_t* pos, int32_t cnt, int32_t& nB);

// 1 sparse SSSP rows, 2 direct rows (complete graph), 3 dense min-plus.
int select_mode(const HostGraph& g, int forceMode, double denseMin);

}  // namespace shdpe
