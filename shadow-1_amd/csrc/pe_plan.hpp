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
//   order 1: nearest-hub cells -- a multi-source Dijkstra from
//            the K highest-degree vertices gives every vertex its closest
//            hub; sources sort by (hub, distance to it), so a batch holds
//            sources that reach the rest of the graph through one hub, and
//            the distance to the hub becomes the lane's bucket key offset
//            (k_batch_rows: a lane's key is dist + maxOff - off).
//   order 2 (default): hub-group cells -- the same hubs in HUB_GROUPS groups
//            (hub_group_distances); sources sort by (nearest hub, nearest
//            hub of another group, the gap between the two, distance to the
//            nearest), so the sources of a batch also agree on the side of
//            the cell they sit on.  rowOff is the nearest-hub distance as in
//            order 1, and `groups` feeds batch_order_cost.
// Scheduling only: results never depend on it (tools/sim/ models the
// schedule: C4 arc visits 3.9 -> 2.2 x m per batch with offsets, dirty
// lanes and a far set at delta = mean arc latency).

// Hub k of degree_order (k < K = min(256, n / 400), at least 1) belongs to
// group k % HUB_GROUPS.
constexpr int HUB_GROUPS = 16;

// Per attached position p and group j, at [p * G + j]: the distance from the
// nearest hub of the group over out-arcs and that hub's rank in degree_order
// (equal distances: the lower rank).  +inf / INT32_MAX where the group is
// empty or no hub of it reaches the vertex.
struct HubGroups {
    int G = 0;
    std::vector<double> dist;
    std::vector<int32_t> hub;
    bool empty() const { return G == 0; }
};
// One multi-source Dijkstra per non-empty group, each over arrays of its own,
// on min(groups, 16, hardware threads) threads (threads > 0: on that many):
// the result does not depend on the thread count.
HubGroups hub_group_distances(const HostGraph& g, const std::vector<int32_t>& attached, int threads = 0);

struct BatchRanks {
    std::vector<int32_t> rank;     // table position -> batch order rank
    std::vector<double> rowOff;    // table position -> distance to its batch hub (orders 1, 2)
    HubGroups groups;              // order 2 only
};
BatchRanks batch_ranks(const HostGraph& g, const std::vector<int32_t>& attached,
                       const std::vector<int32_t>& posOf, int order);

// Batches of LB nearby sources (rank order) out of the cnt positions pos[],
// -1 pads the last; nB = their number.  With rowOff, longest batches first.
std::vector<int32_t> batch_order(const std::vector<int32_t>& rank, const std::vector<double>& rowOff,
                                 int LB, const int32_t* pos, int32_t cnt, int32_t& nB);

// The batches of batch_order (same composition: consecutive LB rows by rank,
// the pads last), sequenced by non-increasing predicted relax cost, equal
// costs in rank order.  A batch's cost, in units of one pass over the arcs:
//   (c0 + cOff * meanOff + cSpread * spread) * lanes present / LB
// with meanOff the lanes' mean rowOff and spread the rms, over the lanes and
// the groups with a finite distance, of (group distance - rowOff) less its
// mean over the batch's lanes in that group -- how far the sources are out of
// step with each other -- both in units of meanArcLatency.  (The constants:
// pe_plan.cpp.)  cost, if given, receives the nB costs in the order returned.
std::vector<int32_t> batch_order_cost(const std::vector<int32_t>& rank, const std::vector<double>& rowOff,
                                      const HubGroups& groups, double meanArcLatency, int LB,
                                      const int32_t* pos, int32_t cnt, int32_t& nB,
                                      std::vector<double>* cost = nullptr);

// 1 sparse SSSP rows, 2 direct rows (complete graph), 3 dense min-plus.
int select_mode(const HostGraph& g, int forceMode, double denseMin);

}  // namespace shdpe
