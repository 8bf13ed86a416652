// pe_plan.hpp -- what shd_pe_create decides on the host before anything is
// uploaded: the device vertex ids (degree relabelling), the batch schedule
// (ranks, hub distances, batch order and, per composed batch, the lanes'
// bucket key offsets), the compute mode and the row-shard plan.
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
//            order 1; `groups` feeds batch_order_cost and lane_offsets, which
//            replaces rowOff as the bucket key offset batch by batch.
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
    std::vector<double> rowOff;    // table position -> distance to its nearest hub (orders 1, 2)
    HubGroups groups;              // order 2 only
};
BatchRanks batch_ranks(const HostGraph& g, const std::vector<int32_t>& attached,
                       const std::vector<int32_t>& posOf, int order);

// Batches of LB nearby sources (rank order) out of the cnt positions pos[],
// -1 pads the last; nB = their number.  With rowOff, longest batches first.
std::vector<int32_t> batch_order(const std::vector<int32_t>& rank, const std::vector<double>& rowOff,
                                 int LB, const int32_t* pos, int32_t cnt, int32_t& nB);

// The bucket key offset of every lane of the composed batches order[nB * LB]
// (table positions, -1 pads), at [b * LB + l]: k_batch_rows relaxes a lane's
// entry in the bucket of dist + maxOff - off, maxOff the batch's largest.
//   kind 0: the nearest-hub distance rowOff[p] (0 without rowOff: order 0);
//   kind 1 (default): the least-squares shift over the hub groups.  With J
//           the groups whose distance is finite for every real lane of the
//           batch, the shifts s that minimise the squared differences of
//           (d[l][j] - s_l) between the lanes, summed over J, are
//             s_l = mean over J of (d[l][j] - mean over the lanes of d[.][j]),
//           and the offset is s_l less the smallest of the batch: computed
//           as (S_l - min S) / |J| with S_l the sum of d[l][j] over J, which
//           is the same number (the lane means cancel) without their rounding.
//           J empty (a lane no hub reaches, or no groups): kind 0's offsets.
// Every offset is finite and >= 0, pads are 0, the smallest of a kind 1 batch
// is exactly 0, and a lane's offset depends on its batch mates but not on
// their sequence in the batch (sums run over the groups ascending, per lane).
std::vector<double> lane_offsets(const HubGroups& groups, const std::vector<double>& rowOff,
                                 const std::vector<int32_t>& order, int LB, int kind = 1);

// The batches of batch_order (same composition: consecutive LB rows by rank,
// the pads last), sequenced by non-increasing predicted relax cost, equal
// costs in rank order.  A batch's cost, in units of one pass over the arcs:
//   (c0 + cOff * meanOff + cSpread * spread) * lanes present / LB
// with meanOff the lanes' mean rowOff and spread the rms, over the lanes and
// the groups with a finite distance, of (group distance - rowOff) less its
// mean over the batch's lanes in that group -- how far the sources are out of
// step with each other -- both in units of meanArcLatency.  (The constants:
// pe_plan.cpp.)  The lane offsets are lane_offsets(..., offsetKind) of the
// composed batches, permuted with them: the sequence does not depend on the
// kind.  laneOff, if given, receives them and cost the nB costs, both in the
// order returned.
// (The constants of the cost, fitted in pe_plan.cpp; pe_plan_dev.hip computes
// the same cost on the device.)
constexpr double COST_C0 = 0.892, COST_OFF = 0.200, COST_SPREAD = 3.363;
std::vector<int32_t> batch_order_cost(const std::vector<int32_t>& rank, const std::vector<double>& rowOff,
                                      const HubGroups& groups, double meanArcLatency, int LB,
                                      const int32_t* pos, int32_t cnt, int32_t& nB,
                                      std::vector<double>* cost = nullptr,
                                      std::vector<double>* laneOff = nullptr, int offsetKind = 1);

// Batches per round of the split batch kernels: a round's batches keep one
// persisted distance array each (perD bytes, the predecessor filter's flag
// bits included) from the relax to the post kernel.  freeB is the device's
// free memory now, rest the bytes of the per-slot scratch still to allocate;
// 12 GiB stay free for what is allocated later, and a round holds at most
// 160 GiB of distance arrays (C4: one round of 13 GB; C5: one round of 131 GB
// beside its 107 GB table).  Never below `slots` (a workgroup indexes its
// scratch by blockIdx; slots <= nBatchesAll except for an empty shard, whose
// one slot stands) and otherwise never above nBatchesAll; without room, one
// batch per round and slot.  testCap > 0 (SHDPE_BATCH_ROUND, tests only)
// bounds the result from above, down to `slots`.
constexpr size_t ROUND_RESERVE_BYTES = (size_t)12 << 30;
constexpr size_t ROUND_DIST_CAP_BYTES = (size_t)160 << 30;
size_t batch_round_size(size_t slots, size_t nBatchesAll, size_t perD, size_t rest, size_t freeB, int testCap);

// 1 sparse SSSP rows, 2 direct rows (complete graph), 3 dense min-plus.
int select_mode(const HostGraph& g, int forceMode, double denseMin);

}  // namespace shdpe
