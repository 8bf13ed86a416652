// C entry points over pe_plan.cpp for tools/sim/plan_eval.py: the batch plan
// the engine would make for a graph and an attached set (ranks, offsets, batch
// sequence, predicted costs, cost features), and the graph as the batch
// kernel sees it (degree-relabelled CSR).  Built with pe_plan.cpp and
// pe_graph.cpp into tools/sim/libplan.so; host only.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "pe_graph.hpp"
#include "pe_plan.hpp"

using namespace shdpe;

namespace {
struct Plan {
    HostGraph g, dev;                 // as given, and relabelled by degree
    std::vector<int32_t> attached, posOf, devOf;
    BatchRanks br;
    int order = 1;
    int offsetKind = 1;               // lane_offsets kind (plan_offset_kind)
    std::vector<double> resid;        // plan_batches: per batch the spread its lane offsets leave
};
}  // namespace

extern "C" {

void* plan_create(int32_t n, int64_t nEdges, int directed, const int32_t* from, const int32_t* to,
                  const double* lat, const double* loss, const int32_t* att, int32_t nAtt, int order) {
    Plan* p = new Plan();
    ShdPeGraphDesc d{n, nEdges, directed, from, to, lat, loss, nullptr};
    if (build_host_graph(&d, &p->g) != SHD_PE_OK) { delete p; return nullptr; }
    p->posOf.assign(n, -1);
    for (int32_t i = 0; i < nAtt; ++i)
        if (p->posOf[att[i]] < 0) { p->posOf[att[i]] = (int32_t)p->attached.size(); p->attached.push_back(att[i]); }
    const std::vector<int32_t> oldOf = degree_order(p->g);
    p->dev = relabel_graph(p->g, oldOf);
    p->devOf.assign(n, 0);
    for (int32_t k = 0; k < n; ++k) p->devOf[oldOf[k]] = k;
    p->order = order;
    p->br = batch_ranks(p->g, p->attached, p->posOf, order);
    return p;
}

void plan_destroy(void* h) { delete (Plan*)h; }

// 1 (default): least-squares lane offsets; 0: nearest-hub distances
void plan_offset_kind(void* h, int kind) { ((Plan*)h)->offsetKind = kind != 0; }

int32_t plan_positions(void* h) { return (int32_t)((Plan*)h)->attached.size(); }
int64_t plan_arcs(void* h) { return ((Plan*)h)->dev.nArcs(); }
double plan_mean_arc_latency(void* h) { return ((Plan*)h)->g.meanArcLatency; }

// rowPtr[n + 1], col[m], lat[m] of the relabelled graph
void plan_csr(void* h, int32_t* rowPtr, int32_t* col, double* lat) {
    const Plan* p = (Plan*)h;
    std::copy(p->dev.rowPtr.begin(), p->dev.rowPtr.end(), rowPtr);
    std::copy(p->dev.col.begin(), p->dev.col.end(), col);
    std::copy(p->dev.lat.begin(), p->dev.lat.end(), lat);
}

// The whole table's batches in the sequence the engine takes them: per lane
// the source's device vertex id (-1 pads) and the bucket offset the engine
// would upload for it (lane_offsets of the plan's kind); per batch the
// predicted cost (order 2; the mean offset in latency units otherwise) and the
// two features of the cost (mean nearest-hub distance, spread against it;
// latency units).  The same spread against the lane offsets -- the residual
// they leave -- is kept for plan_residual_spread.
int32_t plan_batches(void* h, int LB, int32_t* srcs, double* offs, double* cost, double* feat) {
    Plan* p = (Plan*)h;
    const int32_t T = (int32_t)p->attached.size();
    std::vector<int32_t> pos(T);
    for (int32_t i = 0; i < T; ++i) pos[i] = i;
    int32_t nB = 0;
    std::vector<double> c, lo;
    const double unit = p->g.meanArcLatency;
    const std::vector<int32_t> order =
        p->order == 2 ? batch_order_cost(p->br.rank, p->br.rowOff, p->br.groups, unit, LB, pos.data(), T, nB, &c,
                                         &lo, p->offsetKind)
                      : batch_order(p->br.rank, p->br.rowOff, LB, pos.data(), T, nB);
    if (p->order != 2) lo = lane_offsets(p->br.groups, p->br.rowOff, order, LB, p->offsetKind);
    // the features from group distances of this plan's graph whatever the order
    const HubGroups own = p->order == 2 ? HubGroups() : hub_group_distances(p->g, p->attached);
    const HubGroups& hg = p->order == 2 ? p->br.groups : own;
    std::vector<double> d1(T, 0.0);
    for (int32_t i = 0; i < T; ++i) {
        double mn = INFINITY;
        for (int j = 0; j < hg.G; ++j) mn = std::min(mn, hg.dist[(size_t)i * hg.G + j]);
        d1[i] = std::isfinite(mn) ? mn : 0.0;
    }
    p->resid.assign(nB, 0.0);
    for (int32_t b = 0; b < nB; ++b) {
        double off = 0.0, var = 0.0, varLo = 0.0;
        int lanes = 0, terms = 0;
        for (int l = 0; l < LB; ++l) {
            const int32_t q = order[(size_t)b * LB + l];
            srcs[(size_t)b * LB + l] = q >= 0 ? p->devOf[p->attached[q]] : -1;
            offs[(size_t)b * LB + l] = lo[(size_t)b * LB + l];
            if (q >= 0) { off += d1[q]; ++lanes; }
        }
        for (int j = 0; j < hg.G; ++j) {
            double s = 0.0, ss = 0.0, sLo = 0.0, ssLo = 0.0;
            int k = 0;
            for (int l = 0; l < LB; ++l) {
                const int32_t q = order[(size_t)b * LB + l];
                if (q < 0 || !std::isfinite(hg.dist[(size_t)q * hg.G + j])) continue;
                const double x = (hg.dist[(size_t)q * hg.G + j] - d1[q]) / unit;
                const double y = (hg.dist[(size_t)q * hg.G + j] - lo[(size_t)b * LB + l]) / unit;
                s += x; ss += x * x; ++k;
                sLo += y; ssLo += y * y;
            }
            if (k) {
                var += std::max(0.0, ss - s * s / k);
                varLo += std::max(0.0, ssLo - sLo * sLo / k);
                terms += k;
            }
        }
        p->resid[b] = terms ? std::sqrt(varLo / terms) : 0.0;
        feat[2 * b] = lanes ? off / lanes / unit : 0.0;
        feat[2 * b + 1] = terms ? std::sqrt(var / terms) : 0.0;
        cost[b] = p->order == 2 ? c[b] : feat[2 * b];
    }
    return nB;
}

// Per batch of the last plan_batches: the rms, over lanes and groups, of (group
// distance - lane offset) centred per group (latency units).
void plan_residual_spread(void* h, double* out) {
    const Plan* p = (Plan*)h;
    std::copy(p->resid.begin(), p->resid.end(), out);
}

}  // extern "C"
