// pe_device.hpp -- device-side data layout shared by the engine and kernels.
//
// HBM layout (one engine = one device):
//   graph  : CSR of OUT arcs without self-loops, rows sorted by neighbour id
//            (= igraph incidence order); SoA arrays
//            col[i32] lat[f64] rel[f64] (rel = 1.0 - packetloss, topology.c:437).
//            For directed graphs an IN-arc CSR (inCol/inLat/inRel) is kept for
//            the predecessor pass; undirected graphs alias it to the OUT CSR.
//   vertex : vrel[f64] (1 - vertex packetloss, 1.0 when absent/NaN),
//            self-loop latency/rel + hasSelf (the (s,s) hop, topology.c:1469).
//   table  : row-major [T rows][T cols] lat f64 | rel f64 | hops i32 |
//            pred i32 (optional) | flags u8, one array each (TABLE_FIELDS
//            below), row/col order = attached[].
//   scratch: one slot per resident workgroup: dist f64, hops i32, rel f64,
//            pred i32 (+ heap key/idx, index2 for the exact kernel).
#pragma once
#include <stdint.h>

namespace shdpe {

// One out-arc, 16 bytes: a single global_load_dwordx4 per arc.
struct alignas(16) Arc {
    double lat;
    int32_t col;
    int32_t pad;             // DevGraph::arcs: outToIn of the arc (its slot in the head's in-list)
};

// 12-byte packed arc (col, lat as two dwords): one global_load_dwordx3 per
// arc and a single 12-B-per-arc copy of the graph for the sparse kernel's
// relax loop and predecessor pass (smaller L2 footprint than AoS 16 B + SoA).
struct alignas(4) Arc3 {
    int32_t col;
    uint32_t latLo, latHi;
};

struct DevGraph {
    int32_t n;
    int32_t T;                 // unique attached vertices (= targets)
    const int32_t* rowPtr;     // [n+1]
    const int32_t* col;        // [nArcs]
    const double* lat;
    const Arc* arcs;           // [nArcs] AoS copy of (lat, col) (batch kernel)
    const Arc3* arc3;          // [nArcs] packed 12-B (col, lat) for k_sparse_rows
    const double* rel;
    const int32_t* inPtr;      // [n+1] (aliases rowPtr when undirected)
    const int32_t* inCol;
    const double* inLat;
    const double* inRel;
    const int32_t* outToIn;    // out arc u->v  ->  index of that edge in v's IN list
    const double* vrel;        // [n]
    const double* selfLat;     // [n]
    const double* selfRel;     // [n]
    const uint8_t* hasSelf;    // [n]
    const double* selfMinLat;  // [n] the self path's loop (several loops: newest of min latency)
    const double* selfMinRel;  // [n]
    const int32_t* attached;   // [T]
    const uint8_t* isAttached; // [n]
    const uint32_t* heavyBits; // [ceil(n/32)] vertices with degree >= heavyDeg
    const double* flat;        // [nArcs] multigraphs with a slower newest parallel edge
                               // (latFold) only, else null: the newest edge's latency
                               // (path folds, direct paths; `lat` = group minimum)
    const double* srel;        // [nArcs] latFold only: the self path's reliability
    const int32_t* oldId;      // [n] device id -> caller's vertex id (null: identity).
                               // The batched path relabels vertices by degree (rows
                               // keep igraph's incidence order); pred is mapped back
};

// A table holds the contiguous block of rows [rowStart, rowStart + rows) of
// the T x T path table (one device shard, or the whole table); kernels write
// row position r at local row r - rowStart.
struct DevTable {
    double* lat;
    double* rel;
    int32_t* hops;
    int32_t* pred;     // may be null
    uint8_t* flags;
    int64_t T;
    int64_t rowStart;
};

// The table's fields, the one list of them for host code: allocation, every
// copy out of, into and between tables, and the staging layout walk it in
// this order.  (Kernels name the members.)
struct TableField {
    int32_t off;       // of the field's pointer in DevTable
    int32_t esize;     // bytes per table cell
};
constexpr TableField TABLE_FIELDS[5] = {
    {(int32_t)__builtin_offsetof(DevTable, lat), 8},  {(int32_t)__builtin_offsetof(DevTable, rel), 8},
    {(int32_t)__builtin_offsetof(DevTable, hops), 4}, {(int32_t)__builtin_offsetof(DevTable, pred), 4},
    {(int32_t)__builtin_offsetof(DevTable, flags), 1}};

constexpr int64_t table_cell_bytes() {
    int64_t b = 0;
    for (const TableField& f : TABLE_FIELDS) b += f.esize;
    return b;
}

inline unsigned char* table_field(const DevTable& t, const TableField& f) {
    unsigned char* p;
    __builtin_memcpy(&p, reinterpret_cast<const char*>(&t) + f.off, sizeof(p));
    return p;
}

inline void set_table_field(DevTable& t, const TableField& f, void* p) {
    __builtin_memcpy(reinterpret_cast<char*>(&t) + f.off, &p, sizeof(p));
}

// Rows [row0, row0 + rows) (table positions) of every field that both views
// hold: copy(dst, src, bytes, esize) per field, each side's pointer offset by
// its own rowStart and T; stops at the first non-zero return and returns it.
// A view is any DevTable-shaped description of memory, host or device: a
// caller's buffers are one with rowStart = the first position they hold.
template <class Copy>
inline int for_each_field(const DevTable& src, const DevTable& dst, int64_t row0, int64_t rows, Copy&& copy) {
    for (const TableField& f : TABLE_FIELDS) {
        unsigned char* const s = table_field(src, f);
        unsigned char* const d = table_field(dst, f);
        if (!s || !d) continue;
        const int rc = copy(d + (row0 - dst.rowStart) * dst.T * f.esize, s + (row0 - src.rowStart) * src.T * f.esize,
                            rows * src.T * f.esize, (int)f.esize);
        if (rc) return rc;
    }
    return 0;
}

// A staging block as a view: the fields `wanted` holds, nRows rows of each
// from position firstRow, packed back to back from `base`.
inline DevTable stage_view(void* base, int64_t firstRow, int64_t nRows, const DevTable& wanted) {
    DevTable v{};
    v.T = wanted.T;
    v.rowStart = firstRow;
    unsigned char* q = static_cast<unsigned char*>(base);
    for (const TableField& f : TABLE_FIELDS) {
        if (!table_field(wanted, f)) continue;
        set_table_field(v, f, q);
        q += nRows * wanted.T * f.esize;
    }
    return v;
}

// Engine tuning (defaults in the engine; SHDPE_* environment overrides only
// with SHD_PE_DEBUG_ENV, never in a production build of Shadow).
struct Tuning {
    int spThreads = 512, heavyDeg = 64, layout = -1, wgPerCU = 8, kflags = 0;
    double deltaFactor = 16.0;
    int exactHc = 0, exactPerCU = 0;
    int batch = -1, batchLB = 0, batchGrid = 0, batchOrder = 2, batchWpe = 0;
    int relabel = 1;           // batched path: 1 = device ids by descending degree, 0 = as given
    int batchSplit = 1;        // batched path: relax / post as two kernels (predecessors on demand)
    double batchDeltaFactor = 0.75, batchScratchGB = 64.0;
    double denseMin = 0.25, denseBatchGB = 24.0;
    int densePredMi = 2, denseEpochs = 1;
    int debug = 0, streamWgPerCU = 16;
    int tuneLog = 0;           // print shd_pe_tune's per-variant times (no kernel counters)
    int tieCorrupt = 0;        // tests only: 1 / 2 scale one early-stop slot's exported
                               // distances after the relevance scan (exercises the tie-slot
                               // repair); 3 = k_tie_export treats its first slot as violated
    int pathsGroup = 0;        // shd_pe_get_paths: sources per emulation group (0: exactGrid)
    int pathsChunk = 0;        // ... requests per staging chunk (0: 65,536)
    int pathsFast = 1;         // ... 0: no batch / tie / row tier, every source by the grouped emulation
    int loadSort = 1;          // shd_pe_path_load: 0 keeps the caller's request order (no sort by source)
    int tloadTree = 1;         // shd_pe_table_load: 0 = no tree tier, every source by the request route
    int tloadCorrupt = 0;      // tests only: 1 the first source's expected total is off by one, 2 its first
                               // claimed vertex counts as ambiguous (both: the tree tier hands the source on);
                               // the parent tier: 2 its parent words count as invalid, 3 the expected
                               // weighted vertex count of its second check is off by one
    int loadSlots = 2048;      // ... the reduction's LDS table size (rounded down to a power of two in [8, 2048])
    int predFilter = 1;        // on-demand predecessor pass reads only the in-arcs the relax
                               // flagged (0: every in-arc, BatchScratch::arcHit stays null)
    int postSplit = -1;        // split kernels: the post kernel as two (predecessor part,
                               // label part): 1 / 0 forced; -1: one kernel until
                               // shd_pe_tune times both and keeps the faster
    int laneOffset = 1;       // bucket key offsets of a batch's lanes: 1 the least-squares
                               // shift over the hub groups, 0 the nearest-hub distance
    int failWpe = 0;           // tests only: the relax variant of this wave count flags
                               // every batch failed (a miscompiled variant; shd_pe_tune
                               // must not pick it)
    int batchRoundCap = 0;     // tests only: > 0 = at most this many batches per round of the
                               // split kernels (never below the scratch slots): a small
                               // table takes several rounds
    int tieSlotsCap = -1;      // tests only: >= 0 = at most this many tie slots (0: none, the
                               // state of a graph past 2^30 arcs); -1 unchanged
    int devicePlan = 1;        // tests only: 0 = batch order 2's plan by batch_order_cost on the
                               // host (the reference), 1 = by the plan kernels (pe_plan_dev.hip)
};

struct DevScratch {
    double* dist;      // exact kernel: final distance at pop
    int32_t* hops;
    double* rel;
    int32_t* pred;     // IN-arc index of the chosen predecessor edge, -1 none
    double* heapTail;  // exact kernel: heap positions >= hc, per slot heapStride keys (f64)
                       // then heapStride vertex ids (i32) -- 16 B per entry of stride
    int64_t heapStride;  // heap tail entries per slot
    int32_t* index2;   // exact kernel: 0 never reached, 1 popped, >=2 heap pos+2
    int32_t* queue;    // sparse LAYOUT 3: frontier queues, (stride + hcap) per slot
    double* lfold;     // latFold graphs only (else null): the folded latency label
    int64_t stride;    // elements per slot (>= n)
};

// Batched multi-source kernel (pe_batch.hip): one slot per resident
// workgroup; every per-vertex array is [n][LB] (LB sources of the batch
// side by side, so one arc relaxation serves LB sources with one coalesced
// access).
// Per (vertex, lane) labels of the post kernel, one 16-B record: the label
// walks read a parent's reliability, hop count AND its own parent arc with
// one access instead of three (round 5).
struct alignas(16) BLabel {
    double rel;              // reliability product label (< 0 unresolved)
    unsigned long long ha;   // hop label (low 32 bits, -1 unresolved) | chosen IN-arc << 32
                             // (| TIE_AMB; -1 none)
};

struct BatchScratch {
    unsigned long long* D;   // [slot][nStride][LB] f64 bit patterns (dist)
    BLabel* L;               // [slot][nStride][LB] labels + chosen in-arc
    int32_t* queue;          // [slot][nStride] phase candidate list
    int32_t* next;           // next batch to take (device counter, zeroed per launch)
    int64_t nStride;         // >= n, multiple of 64
    uint32_t* bits;          // [slot][2 * words] pending bitmaps when they exceed LDS (gbits)
    int32_t* flags;          // split kernels: per batch of the round, bit 0 = phase cap hit,
                             // bit 1 = the relax wrote the batch's arcHit bits
    const double* laneOff;   // [batch][LB] beside the launch's batchRows: the lane's bucket
                             // key offset (pe_plan.hpp lane_offsets; pads 0), set per launch
    // predecessor filter (split kernels): one bit per in-arc slot -- inPtr /
    // inCol order when directed, the head's own row when undirected -- set by
    // the relax when some lane's pre-check of the arc found dist[u] + w <=
    // dist[x]; the post kernel's on-demand predecessor pass gathers only the
    // flagged in-arcs.  Null: no filter (every in-arc is gathered).  The
    // relax collects a batch's bits in LDS and writes them out at its end
    // (bit 1 of flags[batch]); launch_batch_rows sets hitLds when they fit
    // behind the pending bitmaps in the variant's LDS.
    uint32_t* arcHit;        // [batch of the round][mStride / 32]
    int64_t mStride;         // bits per batch: >= in-arcs, multiple of 128
    int32_t hitLds;          // set per launch (the relax of this variant flags in-arcs)
    unsigned long long* predCnt;   // SHD_PE_DEBUG_COUNTERS only (else null): [0] in-arcs of the
                             // entries the on-demand pass claimed, [1] in-arcs it gathered
    // post kernel in two parts (PART 5 / 6): LB holds one label array per
    // batch of the round ([batch][nStride][LB]; null while the shard runs the
    // one post kernel), and the label part lists the batches that need the
    // unsplit kernel's second attempt: redo[0] = their count in this round
    // (zeroed before each label launch), redo[1] = the count over the call,
    // redo[REDO_LIST ...] = their batch indices.  redoRun (set per launch):
    // PART 2 runs over that list, from the full predecessor pass.
    BLabel* LB;
    int32_t* redo;
    int32_t redoRun;
};
constexpr int REDO_LIST = 16;

struct BatchLaunch {
    int32_t lb;              // sources per batch (8, 16 or 32)
    int32_t threads;         // workgroup size
    int32_t grid;            // resident workgroups (= scratch slots)
    int32_t ldsBytes;
    int32_t wpe;             // waves per SIMD the kernel variant is built for (4 or 8)
    double delta;            // bucket width
    int32_t gbits;           // 1: pending bitmaps in global scratch (n > ~655k vertices)
    int32_t split;           // 1: relax and post as two kernels over rounds of batches
};

// Tie export (pe_batch.hip -> k_exact_rows early stop -> k_tie_write): per
// slot the final distances, the fast-path parents (IN-arc index) with
// TIE_AMB marking entries whose parent the igraph heap decides, and the
// largest tied predecessor distance (the emulation stops past it).
constexpr int32_t TIE_AMB = 1 << 30;
struct TieBuf {
    int32_t cap;             // slots (<= 254: rowAmbig holds 2 + slot; mode 3: <= 4096)
    int32_t* count;          // device slot counter (reset per launch)
    double* D;               // [cap][n]
    int32_t* P;              // [cap][n]
    double* thr;             // [cap]
    int32_t* H;              // [cap][n] k_tie_write hop labels
    double* R;               // [cap][n] k_tie_write reliability labels
    int64_t n;
    // deferred export (k_batch_rows post kernel -> k_tie_export): per slot
    // {batch within its round, lane, source, round}; `round` = the device
    // word the host sets to the round whose post kernel runs (null: the
    // post kernel exports in line, after a full predecessor pass)
    int32_t* req;            // [cap][4]
    int32_t* round;
};

// per-entry flags (mirror SHD_PE_F_* in include/shd_pathengine.h)
constexpr uint8_t F_UNREACHABLE = 0x01;
constexpr uint8_t F_NOEDGE = 0x02;
constexpr uint8_t F_ZEROLAT = 0x04;
constexpr uint8_t F_DIRECT = 0x08;
constexpr uint8_t F_EXACT = 0x10;
constexpr uint8_t F_INVALID = 0x80;   // batched helpers: vertex id out of range

struct SparseLaunch {
    int32_t threads;     // workgroup size
    int32_t grid;        // persistent workgroups (= scratch slots)
    int32_t ldsBytes;    // dynamic LDS
    int32_t qcap;        // light frontier queue capacity
    int32_t hcap;        // heavy (wave-per-vertex) queue capacity
    int32_t heavyDeg;    // degree threshold for the heavy queue
    int32_t layout;      // 2: dist+hops+rowPtr in LDS, 1: dist in LDS, 0: HBM slot,
                         // 3: dist+pending in LDS only (2 rows/CU), queues in HBM
    double delta;        // bucket width
    int32_t kflags;      // kernel variant bits (tuning): 1 col / lat arrays instead of the 12-B arcs in
                         // the relax, 2 unused, 4 nontemporal stores in the row writer, 8 grouped predecessor
                         // pass, 16 / 32 / 48 layout 3 with 2 / 1 / 8 lanes per light vertex
};

// kernels (pe_kernels.hip); all launched on `stream`.
// rowAmbig[i]: 0 fast path, 1 full heap emulation, 2 + k tie data in slot k
// of *dTie (device copy; null disables the export).  noRow (shd_pe_get_paths'
// row tier, nRows <= cfg.grid): no table row is stored; row i's parents stay
// in scratch slot i
void launch_sparse_rows(const DevGraph& g, const DevTable& tab, const DevScratch& sc,
                        const int32_t* dRows, int32_t nRows, uint8_t* dRowAmbig,
                        const SparseLaunch& cfg, int32_t* dDbg, const TieBuf* dTie,
                        void* stream, bool noRow = false);
// dSlots (may be null): per exact row its tie slot (-1 = full emulation);
// rows with a slot stop at the slot's threshold and leave their final
// parents in tie.P for launch_tie_write
// hc: heap positions held in LDS (k_exact_rows, n > exact_soa_max_n());
// forceGlobalHeap: k_exact_rows even when the SoA all-LDS kernel would fit
int exact_bits_bytes(int n);
void launch_exact_rows(const DevGraph& g, const DevTable& tab, const DevScratch& sc,
                       const int32_t* dRows, int32_t nRows, int32_t grid, int32_t hc,
                       bool forceGlobalHeap, const int32_t* dSlots, const TieBuf& tie,
                       long long* dXdbg, void* stream);
int exact_soa_max_n();
// tie rows of dense graphs (mode 3): the same emulation with the popped
// vertex's ~n arcs scanned by a whole 1024-thread workgroup; dList: per grid
// slot `stride` entries of exact_dense_list_bytes()
void launch_exact_dense(const DevGraph& g, const DevTable& tab, const DevScratch& sc,
                        const int32_t* dRows, int32_t nRows, int32_t grid, int32_t hc, void* dList,
                        const int32_t* dSlots, const TieBuf& tie, int32_t* dTake, void* stream);
// early-stop tie slots 0 .. nSlots-1 of dense tie rows (undirected graphs):
// distances, in-arc parents (TIE_AMB where the heap decides) and thresholds
// from the min-plus D / P rows dIdx[k] of table positions dPos[k]
void launch_dense_tie_export(const DevGraph& g, const double* D, const int32_t* P, int64_t n,
                             const int32_t* dIdx, const int32_t* dPos, const TieBuf& tie, int32_t nSlots,
                             void* stream);
int exact_dense_list_bytes();
// tie rows whose ambiguous entries lie on no target's path: thr := -1 (the
// exact kernel then keeps the fast-path parents)
void launch_tie_scan(const DevGraph& g, const int32_t* dRows, const int32_t* dSlots,
                     int32_t nRows, const TieBuf& tie, void* stream);
// rows (dRows) with their tie slots (dSlots): hops / reliability along the
// final parents, row writer
void launch_tie_write(const DevGraph& g, const DevTable& tab, const int32_t* dRows,
                      const int32_t* dSlots, int32_t nRows, const TieBuf& tie, void* stream);
void launch_direct_rows(const DevGraph& g, const DevTable& tab, const int32_t* dRows,
                        int32_t nRows, void* stream);
int sparse_max_threads();
// lanes per light vertex of the k_sparse_rows instantiation that `cfg` launches
int sparse_lanes_per_vertex(const SparseLaunch& cfg);
// batched multi-source sparse path (pe_batch.hip): batchRows = nBatches*lb
// table positions (-1 pads a short batch); rowAmbig[i] != 0 when entry i's
// row has equal-distance predecessor ties (-> k_exact_rows): 1 = full heap
// emulation, 2 + k = tie data exported to slot k of *dTie (device copy of
// the descriptor; null disables the export).
void launch_batch_rows(const DevGraph& g, const DevTable& tab, const BatchScratch& bs,
                       const int32_t* dBatchRows, int32_t nBatches, uint8_t* dRowAmbig,
                       const BatchLaunch& cfg, int32_t* dDbg, const TieBuf* dTie, void* stream,
                       int part = 0);   // (part 4: the post kernel, part 2, storing no table row)
const void* batch_kernel_ptr(int lb, int wpe, bool gbits, int part = 0);
// dynamic LDS of a variant's part (5: bitmaps + heavy list, 6: walk stacks, any
// other: the larger of bitmaps and stacks)
int batch_lds_bytes(int n, int wpe, bool gbits, int part = 0);
// Deferred tie export of one round (after its post kernel): for every slot
// the post kernel requested in round `round`, the tie data of the lane's row
// -- every vertex's distance, its igraph parent (first tight in-arc of
// minimum dist[u], TIE_AMB on equal minima or a zero-increment arc) and the
// tie threshold -- from the round's persisted distance array, over the whole
// GPU; a Bellman violation sends the row to the full emulation (rowAmbig 1;
// violSlot >= 0: tests, that slot's row is treated as violated).
void launch_tie_export(const DevGraph& g, const BatchScratch& bs, int lb, const TieBuf& tie,
                       int round, uint8_t* dRowAmbig, int grid, int violSlot, void* stream);
int batch_threads(int wpe);    // workgroup size of a variant (6 waves: 768, else 1024)
int64_t batch_bits_words(int n);   // per slot, both bitmaps
// whether the relax launched as `cfg` flags in-arcs for the predecessor filter
bool batch_relax_flags(const BatchScratch& bs, const BatchLaunch& cfg, int n);
// batched helpers (pe_aux.hip), all on `stream`
void launch_self_paths(const DevGraph& g, const int32_t* dVerts, int32_t count, int64_t nEdges,
                       double* dLat, double* dRel, uint8_t* dFlags, void* stream);
// mode 0 direct paths (lat, rel, flags), mode 1 adjacency (flags = 0 / 1)
void launch_pairs(const DevGraph& g, const int32_t* dSrc, const int32_t* dDst, int64_t count,
                  int mode, double* dLat, double* dRel, uint8_t* dFlags, void* stream);
void launch_incident_min(const DevGraph& g, const int32_t* dEdgeCount, int32_t* dOut, void* stream);
// path-cache image of a table view -- triangular rows [pv.lo, pv.hi), which
// `tab` holds at local row a - tab.rowStart; the whole table is [0, T) -- in
// the row store's layout (dOff: shd_rowstore_image_layout, all T + 1 entries;
// dImg: the segment from dOff[pv.lo]); dAcc[0] += stored
// entries, dAcc[1] = min stored latency bits (init INF_BITS).  A slot whose
// reverse entry lies in a row >= pv.hi is a need: PACK_S_PENDING in its state
// byte, not in dAcc, counted in dNeedCount[a - pv.lo] (null: a view with no
// rows behind it, nothing counted).  mode 0: the
// non-direct store rule alone; 1: a complete graph's direct table, entries
// stored as direct; 2: the prefersDirectPaths rule (or, `complete`, a complete
// graph whose table holds Dijkstra rows) with adjacency bitmaps in LDS -- g =
// the graph in the caller's ids, dPosOf[n] = vertex -> table position or -1,
// `direct` = also store the direct entries.  -1: mode 2's bitmaps exceed LDS
// (pack_adj_lds_bytes < 0) or its arguments are missing; nothing launched.
int pack_adj_lds_bytes(int64_t T, bool directed);
struct PackView {
    int32_t lo, hi;
};
constexpr uint8_t PACK_S_PENDING = 0x80;   // beside SHD_ROWSTORE_S_*: never in an adopted image
int launch_pack_rowstore(const DevTable& tab, const PackView& pv, const int64_t* dOff, uint8_t* dImg,
                         unsigned long long* dAcc, int32_t* dNeedCount, int mode, const DevGraph* g,
                         const int32_t* dPosOf, bool direct, bool complete, void* stream);
// the needs of the view's rows dRows[0, nRows) (ascending, each with needs) as
// (a, b) int32 pairs, row i's from pair dPre[i] of dPairs, ascending b
void launch_pack_needs(const PackView& pv, int64_t T, const int64_t* dOff, const uint8_t* dImg,
                       const int32_t* dRows, const int64_t* dPre, int32_t nRows, int32_t* dPairs,
                       void* stream);
// per need (a, b) of dPairs, row b in `tab`: ok = the fold (b, a) succeeded, its lat / rel
void launch_pack_answer(const DevTable& tab, const int32_t* dPairs, int64_t n, uint8_t* dOk, double* dLat,
                        double* dRel, void* stream);
// per local row of `tab`: 1 = no F_NOEDGE target (isAllSuccess of topology.c:1815-1859)
void launch_rows_all_success(const DevTable& tab, int32_t rows, int32_t* dOut, void* stream);
// 64-bit fingerprint per table row (local rows firstLocal .. + rows), pe_aux.hip
void launch_row_checksums(const DevTable& tab, int64_t firstLocal, int32_t rows, uint64_t* dOut,
                          void* stream);
// batched path extraction (pe_aux.hip, shd_pe_get_paths); requests are staged
// in chunks of `count`, every array below indexed by the request's place in
// its chunk
struct PathsSizeArgs {
    const int32_t* src;      // [count] caller's vertex ids
    const int32_t* dst;
    int32_t count;
    const int32_t* posOf;    // [n] caller's vertex id -> table position or -1
    int32_t ownLo, ownHi;    // table positions this engine owns (else SHD_PE_ENOTOWNED)
    int32_t rowLo, rowHi;    // ... and this shard: it answers the requests that need one of its rows
    int32_t primary;         // 1: this shard also answers the requests that need no table row
    int32_t complete;        // mode 2: a path is the direct edge
    int32_t* len;            // [count] vertices of the path, 0 with a status (written where this
    int32_t* stat;           // [count]   shard answers; the host presets len 0, stat INT32_MIN)
};
struct PathReq {
    int32_t req;             // request (place in its chunk)
    int32_t slot;            // parent array of its source; -1: [s] or [s, t] as given
    int32_t s, t;            // slot >= 0: DEVICE ids of source and destination; else the caller's
};
struct PathsWalkArgs {
    const PathReq* reqs;
    int32_t nReqs;
    const int32_t* parents;  // [slot][stride] IN-arc of the chosen parent (TIE_AMB masked off)
    int64_t stride;
    int32_t nInArcs;
    const int32_t* len;      // [count]
    const int64_t* off;      // [count + 1] from launch_paths_scan
    int32_t* verts;          // [off[count]] caller's ids, path i at off[i]: [src, ..., dst]
    uint8_t* failed;         // [count] 1: the walk did not arrive at src (nothing of it is a path)
    int32_t* nFailed;
};
// the same walk over one round's persisted distance arrays of the split batch
// kernels (pe_batch.hip): PathReq::slot - slotBase = batch within the round * lb + lane
struct PathsDistArgs {
    const PathReq* reqs;
    int32_t nReqs;
    int32_t lb;
    int32_t slotBase;        // the round's first batch * lb
    const uint8_t* rowAmbig; // the round's [batches * lb] ambiguity bytes (non-zero: handed on)
    const int32_t* len;
    const int64_t* off;
    int32_t* verts;
    uint8_t* failed;         // [count] 1: handed on to the emulation
};
void launch_paths_walk_dist(const DevGraph& g, const BatchScratch& bs, const PathsDistArgs& a, void* stream);
// shd_pe_table_load's tree tier (pe_batch.hip, k_tree_load): the all-pairs load
// of the sources of one round of the split kernels, over the round's persisted
// distance arrays.  Entry i of the round is batch i / lb, lane i % lb.
struct TreeLoadArgs {
    const int32_t* batchRows;   // the round's [nBatches * lb] table positions (-1 pads)
    const uint8_t* rowAmbig;    // the round's ambiguity bytes (non-zero: not started)
    int32_t nBatches, lb;
    const int32_t* attDev;      // [T] table position -> its vertex in the ids of the path kernels' graph
    const uint64_t* weight;     // [nBatches * lb][T] the weight rows of the round's entries; null: 1
    int32_t* par;               // [grid][n * lb] scratch slots: parent in-arc ...
    uint64_t* sum;              // ... subtree sum ...
    int32_t* pend;              // ... children that have not arrived
    int64_t nArcs;
    uint64_t* acc;              // [nArcs + n] caller's ids, as PathsLoadArgs::acc
    uint8_t* handed;            // the round's [nBatches * lb]: 1 = started and handed on after a check
    uint64_t* out;              // [8] added to: totals[0..3] of the sources served, [4] those sources,
                                // [5] entries claimed by them, [6] global adds issued, [7] commit errors
    int32_t corrupt;            // tests: 1 / 2 (SHDPE_TLOAD_CORRUPT) on the round's entry corruptSlot
    int32_t corruptSlot;        // (-1: none)
};
// grid: scratch slots (workgroups) to use, at most
void launch_tree_load(const DevGraph& g, const DevGraph& gAux, const DevTable& tab, const BatchScratch& bs,
                      const TreeLoadArgs& a, int grid, void* stream);
// ... its tree kernel over explicit parent arrays (pe_aux.hip, k_tree_load_parents;
// shd_pe_table_load_set_parent_tier): listed source i has table position pos[i]
// and its parents at parents + slot[i] * stride: IN-arc words as k_paths_walk
// reads them -- the scratch slots k_sparse_rows' row-less form leaves, or the
// tie slots after the early-stop emulation -- or, with vertexIds, the parent's
// vertex id in g's ids: the rows of P the dense predecessor pass leaves
// (launch_dense_rows, DENSE_PRED).
struct TreeParentsArgs {
    const int32_t* pos;         // [nSrc] table positions
    const int32_t* slot;        // [nSrc] parent array of each source; null: source i has slot i
    int32_t nSrc;
    const int32_t* attDev;      // [T] as TreeLoadArgs::attDev
    const int32_t* parents;
    int64_t stride;
    int32_t nInArcs;
    int32_t vertexIds;          // non-zero: parents holds vertex ids, not in-arc words
    const uint8_t* skip;        // [nSrc] or null: non-zero = the source does not run (the sparse rowAmbig,
                                // the dense rowAmb)
    const double* thr;          // by slot, or null: NaN = the slot failed the emulation's check, handed on
    const uint64_t* weight;     // [nSrc][T]; null: 1
    uint64_t* sum;              // [grid][n] scratch slots: subtree sum ...
    int32_t* pend;              // ... children that have not arrived ...
    int32_t* mark;              // ... claimed (1) or not (0)
    int64_t nArcs;
    uint64_t* acc;              // [nArcs + n]
    uint8_t* handed;            // [nSrc] 1 = run and handed on
    uint64_t* out;              // [8] as TreeLoadArgs::out
    int32_t corrupt;            // tests: 1 / 2 / 3 (SHDPE_TLOAD_CORRUPT) on listed source corruptAt
    int32_t corruptAt;          // (-1: none)
};
void launch_tree_load_parents(const DevGraph& g, const DevGraph& gAux, const DevTable& tab,
                              const TreeParentsArgs& a, int grid, void* stream);
// ... and its direct kernel for complete graphs (pe_aux.hip): rows [row0, row0 +
// rows) of the pair matrix, every path [s, t] (or [s]), one thread per pair
struct TableDirectArgs {
    const int32_t* attached;    // [T] caller's ids
    int32_t T, row0, rows;
    const uint64_t* weight;     // [rows][T]; null: 1
    int64_t nArcs;
    uint64_t* acc;              // [nArcs + n]
    uint64_t* out;              // [4] totals, added to
};
void launch_table_direct(const DevGraph& gAux, const TableDirectArgs& a, void* stream);
// the same walk over converged min-plus distance rows (pe_dense.hip), a wave per
// request: PathReq::slot = the source's row of D
struct PathsDenseArgs {
    const PathReq* reqs;
    int32_t nReqs;
    const double* D;         // [rows][ldD]
    int64_t ldD;
    const int32_t* len;
    const int64_t* off;
    int32_t* verts;
    uint8_t* failed;         // [count] 1: handed on to the emulation
};
void launch_paths_walk_dense(const DevGraph& g, const PathsDenseArgs& a, void* stream);
void launch_paths_size(const DevGraph& gAux, const DevTable& tab, const PathsSizeArgs& a, void* stream);
void launch_paths_scan(const int32_t* dLen, int32_t count, int64_t* dOff, void* stream);
// the flag bytes of table rows dRows[0, nRows) to dBuf (nRows x T) or back
void launch_paths_flags(const DevTable& tab, const int32_t* dRows, int32_t nRows, uint8_t* dBuf,
                        bool restore, void* stream);
void launch_paths_walk(const DevGraph& g, const PathsWalkArgs& a, void* stream);
// per output entry the latency and 1 - packetloss of the edge into it (entry
// 0 of a path: 0.0); gAux / dVerts in the caller's ids; either output may be null
void launch_paths_hops(const DevGraph& gAux, const int64_t* dOff, int32_t count, int64_t entries,
                       const int32_t* dVerts, double* dHopLat, double* dHopRel, int32_t* dNFailed,
                       void* stream);
// shd_pe_path_load's reduction over the same staging: per output entry the weight
// of its request added to acc[nArcs + vertex] and, past a path's first entry, to
// acc[arc into it]
struct PathsLoadArgs {
    const int64_t* off;      // [count + 1]
    int32_t count;
    int64_t entries;         // off[count]
    const int32_t* verts;    // [entries] caller's ids
    const uint64_t* weight;  // [count]
    int64_t nArcs;
    uint64_t* acc;           // [nArcs + n] sums mod 2^64
    int32_t* nFailed;        // an entry that is no vertex, a hop without an arc
    int32_t slots;           // size of the workgroup's LDS table (rounded down to a power of two in [8, 2048])
    uint64_t* nIssued;       // debug counters (else null): global atomic adds issued
};
void launch_paths_load(const DevGraph& gAux, const PathsLoadArgs& a, void* stream);
// dense path (pe_dense.hip)
// launch_dense_rows' stages: everything (sweeps, predecessor pass, row writer);
// the sweeps to convergence alone, which leave the distance rows in D and
// touch neither P, rowAmb nor the table (shd_pe_get_paths' row tier); or the
// sweeps and the predecessor pass without the row writer, which leave D, the
// parent rows in P and the tie bytes in rowAmb for the caller and do not touch
// the table (shd_pe_table_load's parent tier)
enum DenseStage { DENSE_ALL = 0, DENSE_SWEEPS = 1, DENSE_PRED = 2 };
void launch_dense_build(const DevGraph& g, double* W, double* Rl, int64_t n, int64_t nArcs,
                        void* stream);
int launch_dense_rows(const DevGraph& g, const DevTable& tab, const double* W, const double* Rl,
                      double* D, int32_t* P, uint8_t* rowActive, uint8_t* rowChanged,
                      uint8_t* rowAmb, int32_t* dAny, uint8_t* chunkEpoch, const int32_t* dRows,
                      int32_t nRows, int64_t n, const Tuning& tu, void* stream, int* sweepsOut,
                      double* flopsOut, DenseStage stage);

}  // namespace shdpe
