// pe_engine.hpp -- the engine's host state, shared by pe_engine.hip (create,
// configure, compute, tune, paths) and pe_rows.hip (row transport).  What create
// decides on the host alone -- device ids, batch schedule, mode, shard plan --
// is pe_plan.hpp, free functions that take no engine state.  Private to the
// library: nothing here is part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <atomic>
#include <memory>
#include <mutex>
#include <vector>

#include "pe_device.hpp"
#include "pe_graph.hpp"
#include "pe_plan.hpp"
#include "shd_pathengine.h"

namespace shdpe {

// A shard's choice of k_batch_rows variant.  configure_batch fills it,
// ensure_batch lowers every grid in it to the scratch slots (the one place: a
// workgroup indexes its slot by blockIdx), shd_pe_tune times cand[] and
// writes the picks.  Every launch of the batched path takes its BatchLaunch
// from relax / post or from a BatchTrial of the tune.
struct BatchPlan {
    BatchLaunch cand[4];            // what shd_pe_tune times, in its order: the untuned relax
                                    // pick, the other of 4 / 8 waves, 6 waves
    BatchLaunch candPred[4], candLabel[4];   // cand[k] as the post kernel's two parts (PART 5 / 6):
                                    // the part's own LDS bytes and grid
    int nc = 0;
    BatchLaunch relax{};            // picks in use: the relax launch (with the delta chosen) ...
    BatchLaunch post{};             // ... and, split kernels, the post launch: the one post kernel,
                                    // or (postSplit) its predecessor part ...
    BatchLaunch label{};            // ... followed by its label part ...
    BatchLaunch redo{};             // ... and the one post kernel over the batches the label part
                                    // handed back (second attempt: deep trees, undeferred ties)
    bool postSplit = false;
    bool partsOk = false;           // configure_batch: every candidate's two parts fit a CU
    bool tunable() const { return nc > 1; }
};

// One timed run of shd_pe_tune: the launches to use instead of the plan's
// picks, and what the split kernels' relax / post parts took (summed over
// the rounds; 0 when not split).
// Serves two callers: shd_pe_tune's timed trials (timed, msRelax / msPost) and
// the batch tier of shd_pe_get_paths (noTable), both through relax_batched /
// batch_rounds; a plain compute passes no trial.
struct BatchTrial {
    BatchLaunch relax{}, post{}, label{}, redo{};
    bool postSplit = false;         // post = the predecessor part, label / redo as in BatchPlan
    bool timed = false;
    bool noTable = false;           // shd_pe_get_paths: the post kernel stores no table row
    double msRelax = 0.0, msPost = 0.0, msLabel = 0.0;   // (msLabel: label part + redo launch)
};

// The batch plan composed on the device (pe_plan_dev.hip): a shard's copy of
// what batch_order_cost reads -- uploaded where the host versions are made,
// at create -- and the scratch of the plan kernels (ensure_batch).
struct DevPlan {
    int32_t* rank = nullptr;        // [T]
    double* rowOff = nullptr;       // [T]
    double* hubDist = nullptr;      // [T][G], HubGroups::dist
    int32_t T = 0, G = 0;
    double unit = 1.0;              // batch_order_cost's latency unit
    // scratch: null until ensure_batch ran
    uint32_t *keyIn = nullptr, *keyOut = nullptr;   // [capRows] ranks of the positions, unsorted / sorted
    int32_t* sorted = nullptr;      // [capRows] positions by rank
    int32_t* rowsTmp = nullptr;     // [capRows + 64] composed batches before sequencing ...
    double* offTmp = nullptr;       // ... and their lane offsets
    double *cost = nullptr, *costSorted = nullptr;  // [capBatches]
    int32_t *idx = nullptr, *perm = nullptr;        // [capBatches] batch indices, unsorted / by descending cost
    void* temp = nullptr;           // the sorts' temporary storage
    size_t tempBytes = 0;
    int32_t capRows = 0, capBatches = 0;
    bool inputs() const { return hubDist != nullptr; }
    bool ready() const { return temp != nullptr; }
};

// The words of a batched call that k_plan_emit sets in place of the host's
// memsets (null / 0: not there).
struct PlanControl {
    int32_t* next = nullptr;                 // BatchScratch::next
    int32_t* redo = nullptr;                 // BatchScratch::redo [0], [1]
    unsigned long long* predCnt = nullptr;   // BatchScratch::predCnt [0], [1]
    int32_t* tieCount = nullptr;             // TieBuf::count [0]
    int32_t* tieReq = nullptr;               // TieBuf::req, every word to -1 (round -1)
    int64_t tieReqWords = 0;
    int32_t* dbg = nullptr;                  // the batches' debug counters, zeroed
    int64_t dbgWords = 0;
};

// pe_plan_dev.hip
// bytes of temporary storage for calls of up to maxRows rows in maxBatches batches (0: query failed)
size_t plan_dev_temp_bytes(int32_t maxRows, int32_t maxBatches);
// The plan of the cnt positions at dPos (device) into dBatchRows / dLaneOff and
// the control words, all on `st`; nothing waits on the host.
int launch_plan_dev(const DevPlan& dp, const int32_t* dPos, int32_t cnt, int32_t LB, int32_t kind,
                    int32_t* dBatchRows, double* dLaneOff, const PlanControl& ctl, hipStream_t st);

// shd_pe_get_path: PathsWalkArgs' arrays for one request (off = 0); the path's vertices follow.
struct PathOne {
    int64_t off;
    int32_t len, nFailed;
    PathReq req;
    uint8_t failed, pad[31];
};

struct Shard {
    int gindex = 0;                 // global shard index
    int device = 0;
    int numCUs = 256;
    int32_t rowStart = 0, rowCount = 0;   // table positions owned
    hipStream_t stream = nullptr;
    hipStream_t copyStream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, evA = nullptr, evB = nullptr;
    hipEvent_t evP[4] = {nullptr, nullptr, nullptr, nullptr};   // per-part timing (shd_pe_tune)
    std::vector<void*> allocs;
    DevGraph dg{};                  // path kernels (device ids, possibly relabelled)
    DevGraph dgAux{};               // caller's ids, rows sorted by id (aux kernels)
    DevTable tab{};                 // this shard's rows
    DevScratch sc{};
    bool tableReady = false;
    int32_t* dRows = nullptr;
    uint8_t* dRowAmbig = nullptr;
    int32_t* dDbg = nullptr;
    int32_t pathSrc = -1;           // source whose full parent array sits in exact slot 0
    PathOne* dPath = nullptr;       // shd_pe_get_path's one-request staging, its n vertices behind it
    int32_t rowsCap = 0;
    SparseLaunch cfg{};
    int exactGrid = 0, exactHc = 1;
    BatchPlan plan{};
    int64_t predClaimed = 0, predGathered = 0;   // shd_pe_pred_filter_counts (debug counters)
    bool postSplitOk = false;       // ensure_batch: label arrays per batch (the post kernel may run in two parts)
    int64_t redoBatches = 0;        // shd_pe_post_split_info: batches that took the redo launch
    bool tuned = false;
    BatchScratch bsc{};
    bool batchReady = false;
    int32_t batchRound = 0;         // split kernels: batches per round (persisted dist arrays)
    int32_t batchSlots = 0;         // scratch slots allocated (ensure_batch: no grid of the plan exceeds it)
    int64_t roundsRun = 0, batchesRun = 0;   // shd_pe_batch_info: batch_rounds' rounds and their batches (table passes)
    int32_t* dBatchRows = nullptr;
    double* dLaneOff = nullptr;     // per entry of dBatchRows its lane's bucket key offset
    DevPlan dplan{};                // batch order 2: the plan's inputs and scratch on the device
    uint8_t* dBatchAmb = nullptr;
    TieBuf tie{};                   // early-stop tie rows (batched path)
    int32_t* dSlots = nullptr;      // per exact row its tie slot, -1 full emulation
    TieBuf* dTie = nullptr;         // device copy of `tie` (k_batch_rows reads it)
    int32_t* dDenseIdx = nullptr;   // dense early-stop tie rows: their row of the D / P matrices
    long long* dXdbg = nullptr;     // exact-kernel counters (SHD_PE_DEBUG_COUNTERS)
    bool tieTried = false;
    double *dW = nullptr, *dRl = nullptr, *dD = nullptr;
    int32_t* dP = nullptr;
    uint8_t *dRowA = nullptr, *dRowB = nullptr, *dRowAmbD = nullptr, *dChunkEpoch = nullptr;
    unsigned char* dXList = nullptr;   // k_exact_dense: per slot its pushes / modifies of a pop
    int32_t* dAny = nullptr;
    int32_t denseRows = 0;
    int32_t* dPosOf = nullptr;      // vertex -> table position (caller's ids, as dgAux):
                                    // uploaded by the first prefer-direct fill under copyMu
                                    // (not in `allocs`, which the compute lock guards)
    DevTable full{};                // whole table on this device after gather
    bool fullOwner = false;         // first shard on its device owns `full`
    ncclComm_t comm = nullptr;      // in-process communicator (distinct devices)
    ShdPeStats stats{};
};

}  // namespace shdpe

struct ShdPe {
    shdpe::HostGraph hg;
    std::vector<int32_t> attached;   // unique, first-occurrence order
    std::vector<int32_t> posOf;      // vertex -> table position or -1
    ShdPeOptions opt{};
    shdpe::Tuning tu{};
    int mode = 1;
    bool batched = false;
    std::vector<int32_t> rank;       // table position -> batch order rank
    std::vector<double> rowOff;      // table position -> distance to its nearest hub (orders 1, 2)
    shdpe::HubGroups hubGroups;      // batch order 2: what batch_order_cost and lane_offsets work from
    std::vector<int32_t> devOf;      // caller vertex id -> device id (empty: identity)
    int G = 1;                       // global row shards
    std::vector<int32_t> bounds;     // G + 1 position bounds
    int firstShard = 0;              // global index of shards[0]
    std::vector<std::unique_ptr<shdpe::Shard>> shards;
    std::unique_ptr<std::atomic<uint8_t>[]> rowDone;
    bool gathered = false;
    int64_t putRows = 0;             // distinct rows imported by shd_pe_put_rows (host transport)
    std::vector<uint8_t> putSeen;    // per table row: imported already (a repeated put counts once)
    bool putInit = false;            // own shard rows copied into the full table
    ncclComm_t xcomm = nullptr;      // cross-process communicator (shd_pe_comm_init)
    int32_t ownStart = 0, ownEnd = 0;
    unsigned char* stage[2] = {nullptr, nullptr};   // pinned host staging (portable)
    size_t stageBytes = 0;
    std::mutex mu;                   // compute / gather
    std::mutex copyMu;               // staging buffers
    double msGather = 0.0;
    int64_t pathsInfo[7] = {0, 0, 0, 0, 0, 0, 0};   // shd_pe_paths_info of the last shd_pe_get_paths
    bool pathsRowTier = false;       // shd_pe_paths_set_row_tier
    int64_t loadInfo[2] = {0, 0};    // shd_pe_path_load_info of the last shd_pe_path_load
    int64_t tloadInfo[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // shd_pe_table_load_info of the last shd_pe_table_load
    bool tloadParentTier = false;    // shd_pe_table_load_set_parent_tier
};

#define HIPCHK(x)                                   \
    do {                                            \
        if ((x) != hipSuccess) return SHD_PE_EHIP;  \
    } while (0)

namespace shdpe {

// `count` elements of T on the shard's device, freed with the shard.
template <class T>
int dev_alloc(Shard* s, T** p, size_t count) {
    size_t bytes = count * sizeof(T);
    if (bytes == 0) bytes = 16;
    if (hipMalloc(reinterpret_cast<void**>(p), bytes) != hipSuccess) { *p = nullptr; return SHD_PE_ENOMEM; }
    s->allocs.push_back(*p);
    return SHD_PE_OK;
}

// pe_engine.hip, for the row transport
// the field arrays of a table of `rows` rows at position 0 (pred only with storePred)
int alloc_table(Shard* sh, DevTable& t, size_t rows, size_t T, bool storePred);
int ensure_table(ShdPe* pe, Shard* sh);
int ensure_rows(ShdPe* pe, int32_t start, int32_t count);   // compute what is owned here and missing
int compute_positions_locked(ShdPe* pe, const int32_t* pos, int32_t count);   // caller holds pe->mu
bool row_done(const ShdPe* pe, int32_t p);
Shard* owner_of(ShdPe* pe, int32_t p);
float elapsed(hipEvent_t a, hipEvent_t b);

}  // namespace shdpe
