/*
 * shd_pathengine.h -- C-ABI of the MI355X-native Shadow path engine.
 *
 * Drop-in boundary for Shadow v1.14.0 src/main/routing/topology.c.  The
 * engine replaces the region topology.c:1681-1866 inside
 * _topology_computeSourcePaths (target collection, the igraph Dijkstra call at
 * :1765 and the per-target _topology_computePathProperties fold at :1805-1864):
 * one call returns the dense row for a source, and host C keeps calling
 * _topology_storePathInCache (:1855) per target, so the cache rules, the
 * min-latency/lookahead update (:1375-1385) and logging are unchanged.
 *
 * Plain C types only (no HIP/torch types).  All functions return 0 on success
 * or a negative SHD_PE_E* code; shd_pe_strerror() names it.  Caller-owned
 * input arrays are only borrowed for the duration of the call.  The engine
 * owns its device memory and stream; nothing it returns outlives
 * shd_pe_destroy().  The engine never calls back into topology.c.
 *
 * Threading: compute / gather calls serialise on an engine mutex (the
 * reference holds graphLock around the igraph call, topology.c:1747-1781);
 * shd_pe_get_row / get_rows may be called from any number of threads at any
 * time (a row not yet computed is computed under that mutex first; the
 * computed-row flags are acquire/release atomics).
 *
 * Multi-GPU: the T table rows are split into G contiguous
 * row shards.  One engine owns nDevices of them (one per device, computed
 * concurrently); with shardCount > 1 several engines -- one per process --
 * own the rest.  shd_pe_gather assembles the whole table on every device
 * with RCCL over xGMI (shd_pe_comm_init joins the processes).
 */
#ifndef SHD_PATHENGINE_H
#define SHD_PATHENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SHD_PE_ABI_VERSION 16  /* 7: graph property check (shd_pe_graph_props);
                                  8: fill from row shards (shd_pe_fill_rowstore_shards);
                                  9: shd_pe_pred_filter_counts;
                                  10: shd_pe_create_built (graph build on the device),
                                      shd_pe_graph_digest;
                                  11: shd_pe_post_split_info;
                                  12: shd_pe_batch_info;
                                  13: shd_pe_paths_set_row_tier, shd_pe_paths_info's
                                      info[6];
                                  14: shd_pe_path_load, shd_pe_path_load_info, shd_pe_num_arcs,
                                      shd_pe_arc_list, shd_pe_find_arc, shd_topology_link_load;
                                  15: shd_pe_sparse_info;
                                  16: shd_pe_table_load, shd_pe_table_load_info;
                                      later under 16: shd_pe_table_load_set_parent_tier,
                                      shd_pe_table_load_info's info[8..11];
                                      later under 16: the parent tier serves the dense mode
                                      (no new symbol, no new info entry) */

/* ---- error codes ------------------------------------------------------ */
#define SHD_PE_OK            0
#define SHD_PE_EINVAL       -1   /* bad argument / graph fails topology.c checks  */
#define SHD_PE_ENOMEM       -2   /* host or device allocation failed              */
#define SHD_PE_ENODEV       -3   /* no usable gfx950 device / HIP init failed     */
#define SHD_PE_EUNREACHABLE -4   /* (per entry, see flags) target not reachable    */
#define SHD_PE_ENOSELFLOOP  -5   /* (per entry, see flags) (s,s) self-loop missing */
#define SHD_PE_EMULTI       -6   /* reserved (before round 5: a multigraph whose newest parallel edge is not a fastest one; every multigraph is supported now) */
#define SHD_PE_EHIP         -7   /* HIP runtime error during compute               */
#define SHD_PE_ENOTATTACHED -8   /* vertex is not in the attached set              */
#define SHD_PE_ENOEDGE      -9   /* direct path requested but (s,t) has no edge    */
#define SHD_PE_ENOTOWNED   -10   /* row lives in another engine's shard (gather)   */
#define SHD_PE_ETOOBIG     -11   /* graph exceeds the engine's kernel limits (int32
                                    arc / entry indices; no vertex-count cap since
                                    the pending bitmaps spill to HBM past ~655k)   */
#define SHD_PE_ECOMM       -12   /* RCCL communicator missing or failed            */

/* ---- per-entry flags (uint8) ------------------------------------------ */
#define SHD_PE_F_UNREACHABLE 0x01u /* igraph could not reach t: not stored         */
#define SHD_PE_F_NOEDGE      0x02u /* a hop (t==s: the self-loop) has no edge,
                                      topology.c:1490-1495: not stored            */
#define SHD_PE_F_ZEROLAT     0x04u /* latency 0 replaced by 1 (topology.c:1848)    */
#define SHD_PE_F_DIRECT      0x08u /* entry is a direct edge (isDirect=TRUE)       */
#define SHD_PE_F_EXACT       0x10u /* row had equal-distance predecessor ties and
                                      was resolved by the on-GPU igraph-heap kernel */
#define SHD_PE_F_FAILED (SHD_PE_F_UNREACHABLE | SHD_PE_F_NOEDGE)
#define SHD_PE_F_INVALID     0x80u /* batched helpers: vertex id out of range      */

/* ---- graph description (built once by host C from igraph) ------------- */
/* Edges in igraph edge-id order (GraphML document order), endpoints as
 * returned by igraph_edge(); latency/packetLoss are the 'latency' and
 * 'packetloss' edge attributes (EANV).  vertexPacketLoss is the optional
 * vertex 'packetloss' attribute (VANV) or NULL when the attribute is absent;
 * NaN entries mean "value absent" (topology.c:330-349). */
typedef struct ShdPeGraphDesc {
    int32_t nVertices;
    int64_t nEdges;
    int32_t directed;
    const int32_t* edgeFrom;
    const int32_t* edgeTo;
    const double* edgeLatency;
    const double* edgePacketLoss;
    const double* vertexPacketLoss;
} ShdPeGraphDesc;

/* ---- engine options ---------------------------------------------------- */
#define SHD_PE_DEBUG_ENV      0x1  /* read SHDPE_* tuning variables (never in Shadow) */
#define SHD_PE_DEBUG_COUNTERS 0x2  /* per-launch kernel counters on stderr          */

typedef struct ShdPeOptions {
    int32_t device;          /* first HIP device ordinal                          */
    int32_t batchRows;       /* reserved, 0                                       */
    double delta;            /* delta-stepping bucket width (ms); 0 = auto        */
    int32_t storePred;       /* keep a predecessor-vertex column in the table      */
    int32_t forceMode;       /* 0 auto, 1 sparse delta-stepping, 2 direct gather,
                                3 exact igraph-heap kernel for every row (tests),
                                4 dense blocked min-plus,
                                5 batched multi-source delta-stepping             */
    int32_t nDevices;        /* row shards in this engine, one per device; 0 = 1 */
    const int32_t* devices;  /* NULL: device, device+1, ...; else nDevices ordinals
                                (a repeated ordinal = several logical shards on
                                one device, e.g. to test sharding on one GPU)    */
    int32_t shardIndex;      /* multi-process: this engine's index ...            */
    int32_t shardCount;      /* ... among shardCount engines (0 or 1: all rows)   */
    int32_t debugFlags;      /* SHD_PE_DEBUG_*                                    */
} ShdPeOptions;

typedef struct ShdPe ShdPe;

/* Engine statistics (cumulative since create / reset). */
typedef struct ShdPeStats {
    int64_t rowsComputed;
    int64_t rowsExact;         /* rows resolved by the exact igraph-heap kernel   */
    int64_t arcsRelaxed;       /* sum over rows of m_arcs (frozen metric formula) */
    double msSparseKernel;     /* device time of the delta-stepping kernel        */
    double msExactKernel;      /* device time of the exact (tie) kernel           */
    double msDirectKernel;     /* device time of the direct-gather kernel         */
    double msTotal;            /* device time of whole compute calls              */
    int64_t launchesSparse, launchesExact, launchesDirect;
    int32_t mode;              /* 1 sparse, 2 direct (complete graph), 3 dense     */
    int32_t isComplete;        /* _topology_isComplete() of the graph              */
    int32_t nVertices;
    int64_t nArcs;             /* non-loop arcs (undirected edge = 2 arcs)         */
    int32_t nAttached;
    double deltaUsed;
    double msDenseKernel;      /* device time of the dense min-plus path           */
    int64_t launchesDense;
    int64_t denseSweeps;       /* min-plus sweeps (incl. the confirming one)       */
    double denseFlops;         /* executed min-plus work: 2 per (s,u,v) visited,
                                  sweeps (skipped K chunks excluded) + pred pass */
    int32_t batched;           /* mode 1 runs k_batch_rows (multi-source batches)  */
    int32_t batchLanes;        /* sources per batch (LB) when batched              */
    int32_t nShards;           /* row shards (devices) in this engine              */
    double msGather;           /* device time of shd_pe_gather                     */
    int64_t rowsTieEarly;      /* of rowsExact: early-stop emulation (distances,
                                  parents and the tie threshold exported by the
                                  sparse / batch kernels or, dense path,
                                  k_dense_tie_export; k_tie_write wrote the row) */
    int32_t batchWaves;        /* k_batch_rows variant in use: waves per SIMD (4,
                                  6 or 8; shd_pe_tune picks the faster); with the
                                  split kernels, the relaxation kernel's          */
    int32_t batchPostWaves;    /* split kernels: the post kernel's variant (the
                                  tune times relax and post separately)           */
    int64_t rowsTieRepaired;   /* early-stop tie rows whose exported slot failed the
                                  exact kernel's distance cross-check and were
                                  recomputed by the full emulation (0 when correct) */
    int32_t batchCoop;         /* reserved, always 0 (cooperative relax, retired) */
    int64_t relaxCoopAborts;   /* reserved, always 0 (cooperative relax, retired) */
} ShdPeStats;

/* Defaults for ShdPeOptions. */
void shd_pe_default_options(ShdPeOptions* opt);

/* Build the engine: validates the graph like _topology_checkGraphEdges
 * (latency > 0, packetloss in [0,1]; topology.c:1041-1124), builds the
 * CSR in igraph incidence order, uploads it, and fixes the target set =
 * attached[] (verticesWithAttachedHosts, topology.c:1525-1543; duplicates
 * removed, first occurrence order kept).  Row/column order of the table is
 * the order of the unique attached vertices. */
int shd_pe_create(const ShdPeGraphDesc* graph, const int32_t* attached,
                  int32_t nAttached, const ShdPeOptions* opt, ShdPe** out);

/* ABI 10: the same engine with a choice of who builds its graph.  The device
 * build goes from the edge list (uploaded once, 24 B per edge, through
 * page-locked staging) to the device arrays with kernels and reads the host
 * copy back; for topologies of ~10^8 edges, where the host build and its
 * 52 B-per-arc upload are the cost of create.  Every array, on the host and
 * on the device, is byte-identical to the host build's, so every later call
 * answers the same.  shd_pe_create(...) is
 * shd_pe_create_built(..., SHD_PE_BUILD_HOST, NULL, ...).  An unknown
 * graphBuild is SHD_PE_EINVAL before any other work.  No gfx950 device:
 * SHD_PE_ENODEV, never a silent host run (the device build looks for the
 * device before it reads the graph, the host build after). */
#define SHD_PE_BUILD_HOST   0   /* shd_pe_create's build */
#define SHD_PE_BUILD_DEVICE 1   /* device build; hands off to the host form where it must */
#define SHD_PE_BUILD_AUTO   2   /* device build from a measured edge count up (3,126,250:
                                   a complete graph of 2,500 vertices), else host */
typedef struct ShdPeBuildInfo {          /* optional */
    int32_t built;        /* SHD_PE_BUILD_HOST or _DEVICE: what made the graph */
    int32_t handedOff;    /* 1: device build asked for or chosen, host form made it */
    int32_t handOffWhy;   /* 0 none, 1 parallel edges (the merge rules stay on the host),
                             2 vertex count past the kernels' limit (131072; also an edge
                             count past 2^31 - 1) */
    int64_t deviceBytesPeak;             /* temporaries of the build, outputs excluded */
    double  msUpload, msKernels, msReadback, msHostBuild, msCreate;   /* wall ms; msReadback
                             includes the arc latency statistics pass over the read-back arcs */
} ShdPeBuildInfo;
int shd_pe_create_built(const ShdPeGraphDesc* graph, const int32_t* attached, int32_t nAttached,
                        const ShdPeOptions* opt, int32_t graphBuild, ShdPeBuildInfo* info,
                        ShdPe** out);
/* Under SHD_PE_DEBUG_ENV, SHDPE_BUILD_MAXN lowers the vertex limit of the
 * device build (tests reach the hand-off at a small shape). */

/* Test and diagnosis helper: one 64-bit digest per graph array of local shard
 * `shard`.  Each digest is the wrapping sum over the array's elements of
 * splitmix64(bits ^ index * 0x9e3779b97f4a7c15), bits zero-extended; absent
 * arrays digest to 0.  The host arrays are summed on the host, the device
 * arrays by a kernel where they sit.  *count receives the number of entries
 * (64); SHD_PE_EINVAL when cap is smaller.  The order:
 *    0..17  HostGraph: rowPtr col lat rel outToIn inPtr inCol inLat inRel
 *           foldLat selfPathRel vrel selfLat selfRel selfMinLat selfMinRel
 *           hasSelf edgeCount
 *   18      HostGraph's scalars as seven 64-bit words: n, directed, nEdges,
 *           latFold, isComplete, meanArcLatency, minArcLatency
 *   19..40  the shard's graph in the caller's vertex ids (aux kernels), as
 *           DevGraph declares it: rowPtr col lat arcs (two 64-bit words per
 *           arc) arc3 (three 32-bit words per arc) rel inPtr inCol inLat inRel
 *           outToIn vrel selfLat selfRel hasSelf selfMinLat selfMinRel
 *           attached isAttached heavyBits flat srel
 *   41..63  the path kernels' graph where the batched path relabelled it
 *           (else zeros): the same 22 arrays, then oldId */
int shd_pe_graph_digest(ShdPe* pe, int32_t shard, uint64_t* out, int32_t cap, int32_t* count);

void shd_pe_destroy(ShdPe* pe);

const char* shd_pe_strerror(int code);

/* _topology_isComplete (topology.c:450-552) on the uploaded graph. */
int shd_pe_is_complete(const ShdPe* pe);

/* Number of unique attached vertices (T) and their order. */
int32_t shd_pe_num_attached(const ShdPe* pe);
int shd_pe_attached(const ShdPe* pe, int32_t* outVertices);

/* Compute all rows this engine owns (eager batch, e.g. on the first cache
 * miss); every local shard on its own device, concurrently. */
int shd_pe_compute_all(ShdPe* pe);

/* Optional, once, before timed or production use: computes the engine's
 * own rows with each k_batch_rows variant (8 / 6 / 4 waves per SIMD; the
 * relax and post kernels are timed separately and each keeps its faster
 * variant; the chosen relax is also timed at 0.8 x the bucket width and
 * keeps the faster width -- stats.deltaUsed) for later calls (the ranking
 * differs between boxes of the same SKU and between shard sizes).  The
 * table is left fully computed; no-op on other paths. */
int shd_pe_tune(ShdPe* pe);

/* Compute rows for the given sources (vertex ids, must be attached). */
int shd_pe_compute_rows(ShdPe* pe, const int32_t* srcVertices, int32_t count);

/* Compute rows by table position (0..T-1), e.g. a shard [start, start+count). */
int shd_pe_compute_positions(ShdPe* pe, int32_t start, int32_t count);

/* Copy the row of source srcVertex (computing it if needed) into caller
 * buffers of T entries in attached order.  Any pointer may be NULL.
 * lat/rel follow _topology_computePathProperties exactly; hops = edges folded
 * (1 for t == s: the self-loop); pred = vertex before t (-1 for t == s,
 * needs storePred); flags = SHD_PE_F_*.  For a complete graph the row holds
 * the direct-edge values (_topology_lookupDirectPath, topology.c:1877-1927). */
int shd_pe_get_row(ShdPe* pe, int32_t srcVertex, double* lat, double* rel,
                   int32_t* hops, int32_t* pred, uint8_t* flags);

/* Bulk copy of table rows by position [start, start+count) into caller
 * buffers laid out row-major (count x T, attached order), same fields and
 * values as shd_pe_get_row; any pointer may be NULL.  Rows not yet computed
 * are computed first.  Buffers from shd_pe_host_alloc (or otherwise
 * page-locked) receive the DMA directly; pageable buffers are filled through
 * the engine's pinned staging buffers (DMA of the next block overlaps the
 * multi-threaded host copy of the current one).  Either way a host row store
 * filled after shd_pe_compute_all (topology.c's cache inserts, :1805-1864)
 * pays one pass at PCIe rate instead of one synchronous transfer per field
 * per row. */
int shd_pe_get_rows(ShdPe* pe, int32_t start, int32_t count, double* lat, double* rel,
                    int32_t* hops, int32_t* pred, uint8_t* flags);

/* The igraph shortest path from srcVertex to dstVertex (both attached) as
 * the vertex sequence [src, ..., dst] in verts (cap entries), *len = its
 * length: what topology.c builds hop by hop into its path string
 * (_topology_computePathProperties :1449, :1502-1503, logged by
 * _topology_computeSourcePaths :1831-1841).  The table keeps only each
 * target's predecessor, so the first call for a source re-runs igraph's
 * Dijkstra for it on the device (the exact 2-wheap emulation, one wave:
 * milliseconds to ~1 s at 10^5 vertices); later calls for the same source
 * are a device walk until the next compute or emulation of another source.
 * The walk is shd_pe_get_paths' for one request: the length comes from the
 * table's hops, the vertices are written in order, and a walk that does not
 * end on src is SHD_PE_EUNREACHABLE.  src == dst -> [src]; complete
 * graphs -> [src, dst] (_topology_lookupDirectPath).  SHD_PE_ENOTOWNED for a
 * source outside this engine's shard, SHD_PE_EUNREACHABLE, SHD_PE_EINVAL when
 * the path needs more than cap entries. */
int shd_pe_get_path(ShdPe* pe, int32_t srcVertex, int32_t dstVertex, int32_t* verts,
                    int32_t cap, int32_t* len);

/* shd_pe_get_path for `count` (src[i], dst[i]) pairs in one call: what
 * topology.c:1831-1841 logs on every first miss of a source, collected per
 * row.  Path i is exactly what shd_pe_get_path(src[i], dst[i]) returns
 * (src == dst -> [src]; complete graph -> [src, dst]; else igraph's path, ties
 * decided by its heap) and occupies entries [offsets[i], offsets[i+1]) of
 * verts / hopLat / hopRel.  Entry k > 0 of a path carries the latency and
 * 1 - packetloss of the edge verts[k-1] -> verts[k] as _topology_getEdgeHelper
 * returns them for igraph_get_eid's edge (the newest of parallel edges, the one
 * the row's fold used); entry 0 carries 0.0.
 *
 * A request that shd_pe_get_path would refuse does not fail the call: its
 * code goes to status[i] (SHD_PE_EINVAL for an id out of range,
 * SHD_PE_ENOTATTACHED, SHD_PE_ENOEDGE, SHD_PE_ENOTOWNED, SHD_PE_EUNREACHABLE)
 * and its path is empty.  The codes are tested in shd_pe_get_path's order:
 * range, attachment, then src == dst, which is [src] with status 0 whoever
 * owns the row (it needs none; so a sharded, ungathered engine answers
 * SHD_PE_ENOTOWNED for a foreign source only where src != dst), then the
 * complete graph's edge, the owner, and the table's flags.
 * Lengths come from the table alone (hops + 1 for a
 * reachable src != dst); rows not yet computed are computed first, as in
 * shd_pe_get_rows.
 *
 * offsets (count + 1 entries, required) is always filled completely.
 * verts == NULL is the sizing call: nothing else is written, no Dijkstra is
 * re-run, the call returns 0.  offsets[count] > cap: SHD_PE_EINVAL with
 * offsets (and status) still valid.  Otherwise every non-NULL array is filled,
 * per owning shard in tiers (the batch tier and the row tier never both apply):
 *  - batch tier (the batched multi-source path with split kernels, the large
 *    sparse graphs' default): one relax + post pass over the unique requested
 *    sources, which stores no table row; after each round the requests whose
 *    source sits in it are walked over the round's persisted distance arrays,
 *    parent by parent as the post kernel derives them (the tight in-arc of
 *    minimum distance).  A request whose walk meets equal minima is handed on;
 *  - tie tier: the rows that pass gives a tie slot (early-stop tie rows) run
 *    the exact stage's relevance scan and early-stop emulation, which leave
 *    the row's final parents in its slot, and their requests are walked over
 *    those.  A slot that fails the emulation's consistency check, and a walk
 *    that does not arrive at its source, are handed on;
 *  - row tier (off until shd_pe_paths_set_row_tier switches it on; the per-row
 *    sparse kernel and the dense min-plus path, neither latFold nor forceMode
 *    3): one pass of the mode's own relax stage over the unique requested
 *    sources, which stores no table row.  Sparse: in groups of one row per
 *    resident workgroup, each row's parents stay in its workgroup's scratch
 *    slot and the requests of the rows without a tie are walked over them; the
 *    tie rows with a slot go through the tie tier's procedure, group by group.
 *    Dense: the min-plus sweeps alone, in chunks of the dense batch, and one
 *    walk per chunk over the converged distance rows, a wave per request, which
 *    derives each parent as the predecessor pass does (the unique tight in-arc
 *    of minimum distance) and hands the request on where there is none;
 *  - grouped emulation (every mode; what shd_pe_get_path does, wide): igraph's
 *    Dijkstra on the device (the exact heap emulation) for the remaining
 *    unique sources -- rows the pass sends to the full emulation, sources of
 *    requests handed on, and every source where the tiers above do not
 *    apply -- in groups of one row per resident workgroup, one walk launch
 *    per group over all its requests.
 * Only the grouped emulation stores table rows: the values they hold already,
 * with SHD_PE_F_EXACT on every entry until the row's saved flag bytes are put
 * back right after the group's launch.  That flag bit of such a row is the
 * one thing a concurrent shd_pe_get_row(s) can see differ during the call; no
 * other table byte, no computed-row flag and no ShdPeStats field changes.
 * Takes the compute lock. */
typedef struct ShdPePathsOut {      /* any pointer but offsets may be NULL */
    int64_t* offsets;   /* count + 1: path i occupies [offsets[i], offsets[i+1]) */
    int32_t* verts;     /* [src, ..., dst] in the caller's vertex ids          */
    double*  hopLat;    /* same indexing; entry k > 0 of a path = the edge verts[k-1] -> verts[k]; */
    double*  hopRel;    /*   entry 0 of every path = 0.0                        */
    int32_t* status;    /* count: 0 or the SHD_PE_E* code of request i          */
    int64_t  cap;       /* entries available in verts / hopLat / hopRel         */
} ShdPePathsOut;
int shd_pe_get_paths(ShdPe* pe, const int32_t* src, const int32_t* dst, int64_t count,
                     const ShdPePathsOut* out);
/* Of the last shd_pe_get_paths or shd_pe_path_load call (the load call fills
 * them as a shd_pe_get_paths call of the same requests does; ShdPeStats is not
 * touched), the first min(n, 7) of: info[0] unique sources served wholly by the batch tier,
 * info[1] unique sources served wholly from early-stop tie parents (the tie
 * tier), info[2] unique sources served by the grouped full emulation (each
 * unique source with a walk counts in exactly one of info[0], [1], [2] and
 * [6]), info[3] requests that left the batch, the tie or the row tier after
 * its check and were finished by the emulation, info[4] emulation groups
 * launched, info[5] device time of the call from events, in integer
 * microseconds, info[6] (ABI 13) unique sources served wholly by the row tier. */
int shd_pe_paths_info(const ShdPe* pe, int64_t* info, int32_t n);
/* ABI 13.  enable != 0: later shd_pe_get_paths calls may use the row tier
 * where it applies -- an engine on the per-row sparse kernel (mode 1, not
 * batched) or on the dense min-plus path (mode 3), neither a latFold multigraph
 * nor forceMode 3; on every other engine the call succeeds and changes
 * nothing.  Off by default.  (Under SHD_PE_DEBUG_ENV, SHDPE_PATHS_FAST=0 still
 * turns every fast tier off.)  Takes the compute lock; NULL: SHD_PE_EINVAL. */
int shd_pe_paths_set_row_tier(ShdPe* pe, int32_t enable);

/* ---- link and vertex load from path packet counts (ABI 14) -------------
 * The reference leaves two logs for post analysis: each source's paths hop by
 * hop (topology.c:1831-1841) and, at teardown, every cached path with its
 * packet counter (_topology_logAllCachedPaths, :1929-1967, path.c:59-71).
 * shd_pe_path_load is their join, reduced on the device: how much weight
 * crossed each arc and each vertex of the graph.
 *
 * Arcs are the merged non-loop OUT arcs in the caller's vertex ids, sorted by
 * `from`, then by `to`: parallel edges are one arc (igraph_get_eid's edge, the
 * newest, stands for the group), an undirected edge is two arcs, a self-loop
 * is none.  shd_pe_num_arcs is their number (ShdPeStats::nArcs),
 * shd_pe_arc_list writes both endpoint arrays (that many entries each),
 * shd_pe_find_arc gives the index of the arc from -> to, -1 where there is
 * none (ids out of range included), -2 for from == to.  None of the three does
 * device work; NULL: 0 / SHD_PE_EINVAL / -1. */
int64_t shd_pe_num_arcs(const ShdPe* pe);
int shd_pe_arc_list(const ShdPe* pe, int32_t* from, int32_t* to);
int64_t shd_pe_find_arc(const ShdPe* pe, int32_t from, int32_t to);
/* Path i is exactly what shd_pe_get_paths(src[i], dst[i]) returns, with the
 * same status code; w_i = weight[i], or 1 when weight == NULL.
 *   vertexLoad[v] = sum of w_i over the requests with status 0 whose path
 *                   contains v;
 *   arcLoad[a]    = sum of w_i over the hops verts[k-1] -> verts[k] of those
 *                   paths whose arc is a (the arc shd_pe_get_paths reads the
 *                   hop's attributes from; the direction is the path's);
 *   totals[0] requests with status 0, totals[1] sum of w_i * (vertices of path
 *   i), totals[2] sum of w_i * (hops of path i), totals[3] requests with a
 *   non-zero status.
 * So src == dst is the path [src] and adds to vertexLoad[src] only, a complete
 * graph's path is [src, dst], and a request with a non-zero status adds
 * nothing and does not fail the call.  Every non-NULL array is overwritten,
 * not added to; all sums are modulo 2^64.
 *
 * pe or out NULL, count < 0, or count > 0 with src or dst NULL: SHD_PE_EINVAL
 * before anything is written.  Rows not yet computed are computed first.  The
 * requests run through shd_pe_get_paths' chunks and tiers, ordered by the table
 * position of their source (the sums do not depend on the order; a source's
 * pass then runs once, not once per chunk it falls into), and a reduction
 * kernel adds each chunk's staged paths into one accumulator per local shard
 * (64-bit device-scope atomic adds behind a per-workgroup LDS table that sums
 * what shares a place first); no path leaves the device.  (Under
 * SHD_PE_DEBUG_ENV, SHDPE_LOAD_SORT=0 keeps the caller's order and
 * SHDPE_LOAD_SLOTS sizes that table.)  A failed accumulator allocation is
 * SHD_PE_ENOMEM.  Side effects are shd_pe_get_paths': no table byte,
 * computed-row flag or ShdPeStats field changes, the transient SHD_PE_F_EXACT
 * bit of the grouped emulation is the one thing a concurrent reader can see,
 * and shd_pe_paths_info describes the call as it does a shd_pe_get_paths call.
 * Takes the compute lock. */
typedef struct ShdPeLoadOut {      /* any pointer may be NULL */
    uint64_t* arcLoad;    /* shd_pe_num_arcs entries, arc order */
    uint64_t* vertexLoad; /* nVertices entries */
    int32_t*  status;     /* count entries: 0 or the SHD_PE_E* code shd_pe_get_paths gives request i */
    uint64_t* totals;     /* 4 entries, see above */
} ShdPeLoadOut;
int shd_pe_path_load(ShdPe* pe, const int32_t* src, const int32_t* dst,
                     const uint64_t* weight, int64_t count, const ShdPeLoadOut* out);
/* Of the last shd_pe_path_load call, the first min(n, 2) of: info[0] path
 * entries reduced (vertices of all paths), info[1] global atomic adds the
 * reduction issued (counted only under SHD_PE_DEBUG_COUNTERS, else 0). */
int shd_pe_path_load_info(const ShdPe* pe, int64_t* info, int32_t n);

/* ---- all-pairs link and vertex load of a range of source rows (ABI 16) --
 * shd_pe_table_load is shd_pe_path_load of the count * T requests
 * (attached[p], attached[q], w) for p in [start, start + count) and q in
 * [0, T), T = shd_pe_num_attached, w = weight[(p - start) * ld + q] or 1 when
 * weight == NULL: arcLoad, vertexLoad and totals[0..3] are exactly what that
 * call returns (sums modulo 2^64, every non-NULL array overwritten), the path
 * of a pair is shd_pe_get_paths' path, a pair with a status adds nothing and
 * counts in totals[3], and p == q adds to vertexLoad only.  out->status is NOT
 * written: there are count * T requests.  totals come from the table's flags
 * and hops alone, as in shd_pe_path_load, so totals[1] == sum(vertexLoad) and
 * totals[2] == sum(arcLoad) check the kernels against the table.
 *
 * pe, in or out NULL, a range outside [0, T], or weight != NULL with ld < T:
 * SHD_PE_EINVAL before anything is written.  count == 0 is success and writes
 * zeros.  A range that reaches a row another process's engine owns
 * (shardCount > 1, not gathered): SHD_PE_ENOTOWNED before anything is written;
 * a range over several local shards is served shard by shard and summed.  Rows
 * not yet computed are computed first.  Takes the compute lock.  Side effects
 * are shd_pe_path_load's: no table byte, computed-row flag, ShdPeStats field
 * or shd_pe_batch_info counter changes.
 *
 * Three routes serve the sources.  Where shd_pe_get_paths' batch tier applies
 * (the split batch kernels), the tree tier: one pass of those kernels that
 * stores no row, and per round one kernel that seeds every status-0
 * destination of a source with its weight, claims the shortest-path tree
 * upwards from the seeds (each claimed vertex derives its parent once, by the
 * rule shd_pe_get_paths' walks use), sums the subtrees leaves first, checks the
 * source's sum against the expected total and only then adds the sums to the
 * shard's accumulator.  A source with an ambiguous parent, a zero-increment
 * arc, a Bellman violation or an infinite distance on the way, or a failed
 * check, adds nothing there and is handed on.  The weight rows of a round go up
 * through page-locked staging; the count x ld matrix is never on the device as
 * a whole.  On a complete graph one direct kernel adds every pair's edge.
 * Every other source -- tie rows, handed-on sources, engines without the batch
 * tier -- runs shd_pe_path_load's pipeline on requests made inside the call.
 * shd_pe_paths_info and shd_pe_path_load_info afterwards describe that part
 * alone (all zero when there was none).  A failed scratch or staging
 * allocation is SHD_PE_ENOMEM.  (Under SHD_PE_DEBUG_ENV: SHDPE_TLOAD_TREE=0
 * turns the tree tier off; SHDPE_TLOAD_CORRUPT=1 / 2 spoil the first source's
 * expected total / first claimed vertex, tests.)
 *
 * A fourth route, the parent tier, is off until
 * shd_pe_table_load_set_parent_tier switches it on.  It serves sources whose
 * parents stand in an explicit array.  In-arc words: on engines of the per-row
 * sparse kernel, every source from one pass of that kernel that stores no row
 * (groups of at most one row per resident workgroup; the parents stay in the
 * workgroups' scratch slots), and, there and in the batched engines' tree tier,
 * the flagged rows with an early-stop tie slot from the slot's final parents
 * after the relevance scan and the early-stop emulation.  Vertex ids: the dense
 * mode is served from the predecessor pass's parent rows -- per chunk of the
 * dense batch the min-plus sweeps and the predecessor pass run without the row
 * writer, and every row the pass did not flag is summed over its parent row
 * (info[8]); on an undirected graph a chunk's flagged rows take the dense tie
 * slots, the relevance scan and the early-stop emulation as the table's exact
 * stage runs them, and are summed over the slots' final parents (info[9]).
 * One kernel per group seeds, claims upwards over the parents (in-arc words
 * read by shd_pe_get_paths' walk rule: a word that is negative, names no
 * in-arc or has no vertex at its tail fails the source; a vertex id outside
 * [0, n) or equal to its own vertex does too), sums leaves first and commits
 * only after two checks: the source's sum is the expected total, and the sums
 * of all claimed vertices add up to the table's weighted vertex count.  Rows
 * of the full emulation, a tie slot that failed the emulation's consistency
 * check, in the dense mode the flagged rows of a directed graph and those
 * beyond a chunk's tie slots, and every source that fails a check go to the
 * request route.  Not with forceMode 3 or folded latencies.  The accumulator
 * (arcs + vertices, 8 bytes each) is held once on the device and, with the
 * call's sum, twice on the host besides the caller's arrays: 3.2 GB each at
 * 4 x 10^8 arcs.  (Under SHD_PE_DEBUG_ENV:
 * SHDPE_PATHS_FAST=0 turns it off as every fast tier; SHDPE_TLOAD_CORRUPT=1 / 2
 * / 3 spoil the first source's expected total / parent words / expected
 * weighted vertex count in this tier too.) */
typedef struct ShdPeTableLoadIn {
    int32_t start, count;     /* source rows: table positions [start, start+count) */
    const uint64_t* weight;   /* count x ld, row-major: weight[(p-start)*ld + q] is the weight of
                                 (attached[p] -> attached[q]); NULL: 1 for every pair */
    int64_t ld;               /* >= T; ignored when weight == NULL */
} ShdPeTableLoadIn;
int shd_pe_table_load(ShdPe* pe, const ShdPeTableLoadIn* in, const ShdPeLoadOut* out);
/* Switches shd_pe_table_load's parent tier on (enable != 0) or off; off by
 * default.  Takes the compute lock.  pe NULL: SHD_PE_EINVAL.  Independent of
 * shd_pe_paths_set_row_tier. */
int shd_pe_table_load_set_parent_tier(ShdPe* pe, int32_t enable);
/* Of the last shd_pe_table_load call, the first min(n, 12) of: info[0] sources
 * served by the tree tier, info[1] by the direct kernel, info[2] by the request
 * route, info[8] by the parent tier over row parents, info[9] by the parent
 * tier over tie-slot parents (each source in exactly one of the five); info[3]
 * of info[2], sources a tree or parent tier had started and handed on after one
 * of its own checks; info[4] tree entries claimed by the sources of info[0];
 * info[5] device time of the call from events, in microseconds; info[6] rounds
 * the tree tier ran; info[7] global adds its commit issued; info[10] entries
 * claimed by the sources of info[8] and info[9]; info[11] global adds the parent
 * tier's commits issued (info[7], info[11]: SHD_PE_DEBUG_COUNTERS only, else 0). */
int shd_pe_table_load_info(const ShdPe* pe, int64_t* info, int32_t n);

/* Page-locked host memory for shd_pe_get_rows destinations (DMA target, no
 * staging copy).  No reference counterpart: Shadow's row buffers are plain
 * g_new allocations (topology.c:1805-1864). */
int shd_pe_host_alloc(int64_t bytes, void** out);
void shd_pe_host_free(void* p);

/* Copy rows [start, start+count) (table positions) of the device table into
 * caller DEVICE buffers (e.g. an RCCL all-gather staging area).  Row-major,
 * T entries per row.  Any pointer may be NULL.  Rows not yet computed are
 * computed first (as shd_pe_get_rows); rows of another engine's shard need
 * shd_pe_gather first (SHD_PE_ENOTOWNED). */
int shd_pe_copy_rows_device(ShdPe* pe, int32_t start, int32_t count,
                            double* dLat, double* dRel, int32_t* dHops,
                            uint8_t* dFlags);

/* ---- multi-GPU ----------------------------------------- */
/* Global row shards G = shardCount * nDevices and their position bounds
 * (G + 1 entries: shard g owns rows [bounds[g], bounds[g+1])). */
int32_t shd_pe_num_shards(const ShdPe* pe);
int shd_pe_shard_bounds(const ShdPe* pe, int32_t* bounds);
/* The plan itself (host only, no GPU): G contiguous blocks of T rows with
 * equal numbers of `unit`-row work units (16 = one k_batch_rows batch). */
int shd_pe_plan_shards(int32_t T, int32_t G, int32_t unit, int32_t* bounds);
/* Rows this engine owns (the union of its shards, contiguous). */
int shd_pe_owned_range(const ShdPe* pe, int32_t* start, int32_t* count);
/* Assemble the whole T x T table on every device of this engine (computing
 * missing owned rows first): RCCL broadcasts (all-gather with per-shard
 * blocks) over xGMI between distinct devices / processes, device copies
 * between logical shards of one device.  Afterwards every row is readable
 * here.  Multi-process engines need shd_pe_comm_init first. */
int shd_pe_gather(ShdPe* pe);
/* Cross-process RCCL communicator, one rank per engine (nDevices == 1,
 * rank = shardIndex, nranks = shardCount): one process makes the id, the
 * host's own channel (MPI, a socket, torch.distributed) hands its bytes to
 * every process, each calls shd_pe_comm_init.  shardCount 1 is accepted (a
 * one-rank communicator: the gather issues the same RCCL calls, an in-place
 * all-gather of the engine's own rows). */
int shd_pe_comm_unique_id(void* out, int32_t bytes);   /* bytes >= 128 */
int shd_pe_comm_init(ShdPe* pe, const void* uniqueId, int32_t bytes);
/* Host-transport assembly, the alternative to shd_pe_gather where RCCL has no
 * communicator (several ranks on one GPU, a host-only channel between nodes):
 * rows [start, start+count) of ANOTHER engine's shard, received in host
 * buffers (T entries per row, attached order; pred needed iff storePred), are
 * written into this engine's full table.  Multi-process engines only
 * (shardCount > 1, nDevices == 1); own rows -> SHD_PE_EINVAL.  Once every
 * foreign row has arrived, all rows read from the full table as after
 * shd_pe_gather. */
int shd_pe_put_rows(ShdPe* pe, int32_t start, int32_t count, const double* lat, const double* rel,
                    const int32_t* hops, const int32_t* pred, const uint8_t* flags);
/* 64-bit fingerprint of each table row [start, start+count) (computed on the
 * device; own rows, or any row after a gather / put_rows): the wrapping sum
 * over entries j and fields f (lat, rel, hops, flags, pred if stored) of
 * splitmix64(bits ^ (j * 0x9e3779b97f4a7c15 + f * 0xd1b54a32d192ed03)), f =
 * 1..5.  Owners fingerprint their rows before an exchange and every rank the
 * assembled table after it.  No reference counterpart. */
int shd_pe_row_checksums(ShdPe* pe, int32_t start, int32_t count, uint64_t* out);

/* The whole-table path-cache fill in one pass: rows 0..T-1 (computed first
 * if needed -- then the host image is prepared on a host thread while the
 * device computes, so the drop-in's cheapest call is this one alone; a
 * sharded engine must be gathered: SHD_PE_ENOTOWNED) into an EMPTY row store
 * (SHD_PE_EINVAL otherwise, as for unknown fillFlags bits).  The store ends
 * exactly as after this sequence of host calls:
 *   1. shd_rowstore_store_rows over every row in position order, isComplete
 *      from the graph (topology.c:1805-1864 per row); with
 *      SHD_PE_FILL_PREFER_DIRECT its adjacency argument is
 *      adjacent[p][q] = _topology_verticesAreAdjacent(attached[p],
 *      attached[q]) (an arc p -> q; p == q: a self-loop), so the Dijkstra
 *      path of an adjacent pair is refused (:1325-1332), else it is NULL;
 *   2. with SHD_PE_FILL_DIRECT_PAIRS, for every ordered pair (p, q) in
 *      position order, p outer, that topology.c:2019-2021 serves with the
 *      edge itself (complete graph, or PREFER_DIRECT and adjacent) and whose
 *      edge exists: shd_rowstore_store(isDirect = 1) of the
 *      _topology_lookupDirectPath values (:1877-1927), refused where either
 *      direction is cached already.
 * fillFlags == 0 is shd_pe_fill_rowstore (a complete graph stores nothing).
 * The device packs the store's triangular row image
 * (shd_rowstore_image_layout: 17 B per unordered pair instead of 34 B of two
 * rows) and one DMA lands it in page-locked memory the store adopts; the
 * prefer-direct pack keeps one row's adjacency as bitmaps in LDS
 * (SHD_PE_ETOOBIG past 262,144 attached vertices undirected, half that
 * directed -- tables no device holds).  rowResult (optional, T entries): each
 * row's store_row result.  msOut (optional, 3 entries): ms of compute (if
 * any) overlapped with the host image preparation, device pack, DMA. */
struct ShdRowStore;
#define SHD_PE_FILL_PREFER_DIRECT 0x1   /* the graph's preferdirectpaths is true */
#define SHD_PE_FILL_DIRECT_PAIRS  0x2   /* also store the direct entries */
int shd_pe_fill_rowstore_ex(ShdPe* pe, struct ShdRowStore* st, int32_t fillFlags,
                            int32_t* rowResult, double* msOut);
int shd_pe_fill_rowstore(ShdPe* pe, struct ShdRowStore* st, int32_t* rowResult, double* msOut);

/* The same fill from row shards, without a gather (ABI 8).  On an in-process
 * sharded engine (nDevices > 1, repeated ordinals included) every shard packs
 * the image rows of its own table rows on its own device and DMAs that
 * segment to its place in the one host image (distinct devices: concurrently;
 * the image is registered portable).  A slot (a, b > a) whose forward entry
 * is not used wants entry (b, a); where row b is another shard's the slot is
 * a NEED: it is sent to the owner of row b and answered (the fold's success,
 * lat, rel) through pinned host staging, in rounds whose lists stay within
 * needBudgetBytes (<= 0: 64 MiB; 25 B per need; a single image row past the
 * budget gets a round to itself), and the answers are written into the
 * landed image before the store adopts it.  No peer access, no full table on
 * any device, and the engine's gathered state is never set.
 * The store ends byte for byte as shd_pe_fill_rowstore_ex leaves it on the
 * same engine after shd_pe_gather; fillFlags, rowResult and the refusals
 * (SHD_PE_EINVAL for a non-empty store or unknown bits, SHD_PE_ETOOBIG for
 * the prefer-direct LDS limit) are those of _ex.  With one shard, or once the
 * engine is gathered, the call IS _ex (fromFullTable = 1).  An engine that is
 * one of several processes' (shardCount > 1) and not gathered answers
 * SHD_PE_ENOTOWNED: the other rows' store is another process's.
 * The distinct-device path (concurrent PCIe transfers, portable registration)
 * has run on logical shards of one device only: it is unmeasured. */
typedef struct ShdPeFillShardsInfo {
    int32_t shards;          /* table views packed: local shards with rows, or 1 when one full table served the call */
    int32_t fromFullTable;   /* 1: G == 1 or the engine was gathered (the _ex path ran) */
    int64_t needs;           /* slots whose reverse entry lives in another shard's rows */
    int64_t needsStored;     /* of those, answered with a usable reverse entry */
    int64_t needRounds;      /* need-list rounds (0 when needs == 0) */
    int64_t deviceBytesPeak; /* largest per-shard sum of this call's device temporaries */
    double  msCompute, msPack, msResolve, msDma;   /* wall ms, as msOut of _ex, plus the resolve */
} ShdPeFillShardsInfo;
int shd_pe_fill_rowstore_shards(ShdPe* pe, struct ShdRowStore* st, int32_t fillFlags,
                                int64_t needBudgetBytes, int32_t* rowResult,
                                ShdPeFillShardsInfo* info);      /* info optional */

/* Wait for outstanding device work of this engine. */
int shd_pe_synchronize(ShdPe* pe);

/* Measurement helper (not on the path): achievable HBM bandwidth of this
 * engine's device, a 16-B streaming copy of `bytes` (read + write counted),
 * averaged over `iters` launches on the engine's stream; the best of several
 * copy shapes (cache policy, loads in flight, workgroups per CU).  SURVEY.md §8(d)
 * asks for it beside the spec peak; no reference counterpart. */
int shd_pe_stream_bandwidth(ShdPe* pe, int64_t bytes, int32_t iters, double* gbps);

/* Counters of this engine (all its shards).  Both calls take the engine's
 * compute lock: during a running compute they return once it is done.
 * ShdPeStats only grows at its end (ABI 3 added rowsTieRepaired, batchCoop,
 * relaxCoopAborts): a caller
 * built against another header than the library's passes its own
 * sizeof(ShdPeStats) to shd_pe_get_stats_sized, which copies at most that
 * many bytes (the fields both sides know); shd_pe_stats_size() is the
 * library's size.  shd_pe_get_stats writes the library's whole struct. */
int shd_pe_get_stats(const ShdPe* pe, ShdPeStats* out);
int shd_pe_get_stats_sized(const ShdPe* pe, void* out, int64_t outBytes);
int64_t shd_pe_stats_size(void);
int shd_pe_reset_stats(ShdPe* pe);
/* SHD_PE_DEBUG_COUNTERS only (else both 0), cumulative like the stats and
 * reset with them: the in-arcs of the entries the batched post kernel's
 * on-demand predecessor pass claimed, and the in-arcs it gathered -- equal
 * without the predecessor filter, fewer where the relax flagged in-arcs. */
int shd_pe_pred_filter_counts(const ShdPe* pe, int64_t* claimed, int64_t* gathered);
/* The batched post kernel of this process's first shard: *split = 1 when it
 * runs as two kernels (predecessor part, label part), 0 as one; *labelWaves =
 * the label part's waves per SIMD (0 when not split; ShdPeStats.batchPostWaves
 * then names the predecessor part's); *redoBatches = batches, over all
 * shards, that the label part handed to the one post kernel's second attempt
 * since the last shd_pe_reset_stats. */
int shd_pe_post_split_info(const ShdPe* pe, int32_t* split, int32_t* labelWaves, int64_t* redoBatches);
/* The rounds of the split batch kernels on shard `shard` of this process
 * (0 <= shard < shd_pe_num_shards; ABI 12).  A round is the batches whose
 * distance arrays persist from the relax to the post kernel; it is sized at
 * the shard's first batched compute from the free device memory (every table
 * computed so far is one round).  out[0] = batches per round, out[1] = scratch
 * slots (both 0 before that first compute); out[2] = rounds run and out[3] =
 * batches run in them since the last shd_pe_reset_stats, over the computes
 * that write table rows: the timed computes of shd_pe_tune and the pass of
 * shd_pe_get_paths, which put ShdPeStats back as it was, put these back too.
 * A diagnostic of this engine's schedule: it replaces nothing in topology.c,
 * which has no counterpart. */
int shd_pe_batch_info(const ShdPe* pe, int32_t shard, int64_t out[4]);
/* The launch of the per-row sparse kernel as shard `shard` of this process was
 * configured (0 <= shard < shd_pe_num_shards; ABI 15; host only, valid from
 * shd_pe_create on): out[0] = LDS layout (0 row state in HBM, 1 distances in
 * LDS, 2 distances, hops and row pointers in LDS, 3 distances and pending bits
 * only), out[1] = threads per workgroup, out[2] = light queue capacity, out[3]
 * = heavy queue capacity (entries; a frontier beyond either stays pending for
 * the next bucket scan), out[4] = heavy degree threshold, out[5] = lanes per
 * light vertex, out[6] = kernel variant bits, out[7] = persistent workgroups.
 * An engine whose ShdPeStats.batched is 1 runs the batched kernel instead and
 * reports here what the per-row kernel would have run with.  A diagnostic for
 * tests of the SHDPE_* switches (a mistyped one leaves the default, which this
 * call shows): it replaces nothing in topology.c, which has no counterpart. */
int shd_pe_sparse_info(const ShdPe* pe, int32_t shard, int64_t out[8]);

/* ---- batched helpers on the device ------------
 * The per-query lookups below, for many queries in one call: inputs and
 * outputs are host arrays of `count` entries (staged through the engine's
 * device in chunks).  Results are bit-identical to the one-query helpers. */

/* _topology_computeShortestPathToSelf (topology.c:1545-1653) per vertex:
 * lat = 2 * w_min, rel = (1 - loss_min)^2 over v's OUT-incident edges (the
 * first strict minimum in igraph incidence order).  flags[i]:
 * 0, SHD_PE_F_NOEDGE (graph has no edges), SHD_PE_F_INVALID (bad id). */
int shd_pe_self_paths(ShdPe* pe, const int32_t* vertices, int32_t count, double* lat,
                      double* rel, uint8_t* flags);
/* _topology_lookupDirectPath (topology.c:1877-1927) per pair (src[i],dst[i]):
 * flags[i] = SHD_PE_F_DIRECT with lat/rel, SHD_PE_F_NOEDGE (lat = rel = 0),
 * or SHD_PE_F_INVALID. */
int shd_pe_direct_paths(ShdPe* pe, const int32_t* src, const int32_t* dst, int64_t count,
                        double* lat, double* rel, uint8_t* flags);
/* _topology_verticesAreAdjacent (topology.c:1248-1264) per pair: out[i] 1 / 0
 * (0 for an invalid id; s == t is adjacent iff s has a self-loop). */
int shd_pe_adjacent_pairs(ShdPe* pe, const int32_t* src, const int32_t* dst, int64_t count,
                          uint8_t* out);
/* _topology_isComplete (topology.c:450-552) evaluated on the device from the
 * resident CSR: *isComplete = 1 / 0 (agrees with shd_pe_is_complete). */
int shd_pe_is_complete_device(ShdPe* pe, int32_t* isComplete);

/* ---- host-side helpers Shadow keeps in C (no GPU work) ----------------- */
/* _topology_lookupDirectPath (topology.c:1877-1927) for one pair. */
int shd_pe_direct_path(const ShdPe* pe, int32_t s, int32_t t, double* lat, double* rel);
/* _topology_computeShortestPathToSelf (topology.c:1545-1653). */
int shd_pe_self_path(const ShdPe* pe, int32_t v, double* lat, double* rel);
/* _topology_verticesAreAdjacent (topology.c:1248-1264): 1, 0. */
int shd_pe_adjacent(const ShdPe* pe, int32_t s, int32_t t);

/* ------------------------------------------------------------------------
 * Path cache as a dense triangular row store,
 * replacing topology.c's GHashTable<src, GHashTable<dst, Path*>>
 * (_topology_getPathFromCache :1284-1305, _topology_shouldStorePath
 * :1307-1336, _topology_storePathInCache :1338-1386, Path path.c:13-38).
 * Keys are vertex indices of attached vertices; one 25-B slot per unordered
 * pair (the store rule never keeps both directions), remembering the
 * direction it was stored under.  Thread safety: get / increment never lock
 * and may run concurrently with each other and with stores; stores
 * serialise internally.  No GPU work; usable without an engine.
 * ---------------------------------------------------------------------- */
typedef struct ShdRowStore ShdRowStore;

int shd_rowstore_new(int32_t nVertices, const int32_t* attached, int32_t nAttached,
                     ShdRowStore** out);
void shd_rowstore_free(ShdRowStore* st);
/* _topology_getPathFromCache(s, d): 1 and the Path fields if an entry was
 * stored under exactly (s, d), else 0. */
int shd_rowstore_get(const ShdRowStore* st, int32_t s, int32_t d, double* lat, double* rel,
                     int32_t* isDirect, uint64_t* packetCount);
/* _topology_storePathInCache: 1 stored, 0 refused by _topology_shouldStorePath
 * (either direction cached; a non-direct path on a complete graph; a
 * non-direct path for an adjacent pair under prefersDirectPaths -- the caller
 * passes isComplete and preferDirectAndAdjacent), < 0 error. */
int shd_rowstore_store(ShdRowStore* st, int32_t s, int32_t d, int32_t isDirect,
                       int32_t isComplete, int32_t preferDirectAndAdjacent, double lat,
                       double rel);
/* One engine row of source s (T entries in attached order, as shd_pe_get_row
 * returns them) through the per-target loop of topology.c:1815-1859.
 * adjacent (optional): adjacent[j] = prefersDirectPaths && (s, attached[j])
 * is an edge.  Returns 1 if every target succeeded, 0 if not, < 0 error. */
int shd_rowstore_store_row(ShdRowStore* st, int32_t s, const double* lat, const double* rel,
                           const uint8_t* flags, int32_t isComplete, const uint8_t* adjacent);
/* The whole-table fill: `count` engine rows at once (row i of source srcs[i]
 * at lat/rel/flags/adjacent + i * ld, ld >= nAttached -- e.g. a block of
 * shd_pe_get_rows output in shd_pe_host_alloc buffers), with exactly the
 * result of shd_rowstore_store_row on srcs[0], srcs[1], ... in order
 * (topology.c:1805-1864 once per row, in the order Shadow's first misses
 * would have asked for them).  Spread over nThreads host threads (<= 0: up
 * to 16) by slot rows, so no two threads touch one row.  rowResult
 * (optional) receives each row's store_row result (1 all success / 0).
 * Returns 0, or < 0 on error. */
int shd_rowstore_store_rows(ShdRowStore* st, const int32_t* srcs, int32_t count,
                            const double* lat, const double* rel, const uint8_t* flags,
                            int64_t ld, int32_t isComplete, const uint8_t* adjacent,
                            int32_t nThreads, int32_t* rowResult);
/* Bulk fill from a row IMAGE (the engine builds it on the device,
 * shd_pe_fill_rowstore): the store's own row layout, every triangular row a
 * (attached ordinal, len T - a) at offsets[a] from shd_rowstore_image_layout
 * (T + 1 entries, 64-B aligned): SHD_ROWSTORE_IMAGE_HEADER bytes the store
 * fills, lat f64[len], rel f64[len], state u8[len] (SHD_ROWSTORE_S_* bits).
 * Slot k of row a is the unordered pair (a, a + k).  adopt_image hands an
 * image to an EMPTY store (SHD_PE_EINVAL otherwise) with its entry count and
 * minimum stored latency; release(ctx, image) frees it with the store. */
#define SHD_ROWSTORE_IMAGE_HEADER 64
#define SHD_ROWSTORE_S_STORED   0x1u
#define SHD_ROWSTORE_S_DIRECT   0x2u
#define SHD_ROWSTORE_S_REVERSED 0x4u   /* stored under (larger, smaller) ordinal */
int shd_rowstore_image_layout(int32_t T, int64_t* offsets);
int shd_rowstore_adopt_image(ShdRowStore* st, void* image, int64_t bytes,
                             void (*release)(void* ctx, void* image), void* ctx, int64_t stored,
                             double minLatency);
/* topology_incrementPathPacketCounter on a cached entry: 0, or -1 if absent. */
int shd_rowstore_increment(ShdRowStore* st, int32_t s, int32_t d);
int64_t shd_rowstore_size(const ShdRowStore* st);
double shd_rowstore_min_latency(const ShdRowStore* st);
int64_t shd_rowstore_memory_bytes(const ShdRowStore* st);

/* Every cached entry, as stored (src, dst in the stored direction), for the
 * teardown dump (_topology_logAllCachedPaths, topology.c:1929-1967, which
 * walks the two-level GHashTable in hash order; here by smaller attached
 * ordinal).  Not safe against concurrent inserts.  Returns the number of
 * entries visited. */
typedef void (*ShdRowStoreVisit)(int32_t src, int32_t dst, double latency, double reliability,
                                 int32_t isDirect, uint64_t packetCount, void* user);
int64_t shd_rowstore_foreach(const ShdRowStore* st, ShdRowStoreVisit visit, void* user);

/* ------------------------------------------------------------------------
 * Host mirror of the topology.c path API (the drop-in seen by worker.c,
 * tcp.c, host.c): _topology_getPathEntry + the two-level path cache, with
 * rows coming from the engine.  Queries are by vertex index; Shadow's
 * Address -> vertex map (topology.c:1388-1405) stays where it is.
 * ---------------------------------------------------------------------- */
typedef struct ShdTopology ShdTopology;

int shd_topology_new(ShdPe* pe, int32_t prefersDirectPaths, ShdTopology** out);
void shd_topology_free(ShdTopology* top);
/* topology_getLatency / getReliability (topology.c:2065-2087): -1 on error. */
double shd_topology_get_latency(ShdTopology* top, int32_t srcV, int32_t dstV);
double shd_topology_get_reliability(ShdTopology* top, int32_t srcV, int32_t dstV);
/* topology_isRoutable (topology.c:2089-2092). */
int shd_topology_is_routable(ShdTopology* top, int32_t srcV, int32_t dstV);
/* topology_incrementPathPacketCounter (topology.c:2053-2063): 0 / -1. */
int shd_topology_increment_path_packet_counter(ShdTopology* top, int32_t srcV, int32_t dstV);
/* Inspect the cache entry stored under (src,dst): 1 present, 0 absent. */
int shd_topology_cached(const ShdTopology* top, int32_t srcV, int32_t dstV,
                        double* lat, double* rel, int32_t* isDirect, int64_t* packetCount);
double shd_topology_min_latency(const ShdTopology* top);
int64_t shd_topology_cache_size(const ShdTopology* top);
int64_t shd_topology_rows_computed(const ShdTopology* top);
/* The whole cache in one call, before the first query (SHD_PE_EINVAL once the
 * cache holds an entry): shd_pe_fill_rowstore_ex on the mirror's own store
 * with SHD_PE_FILL_DIRECT_PAIRS, plus SHD_PE_FILL_PREFER_DIRECT when the
 * mirror prefers direct paths.  Afterwards every stored pair of an undirected
 * graph is a lock-free hit and no query computes a row; on a directed graph
 * a pair stored under its reverse key still takes the miss path once, which
 * re-probes that key.  msOut (optional, 3 entries) as shd_pe_fill_rowstore. */
int shd_topology_fill(ShdTopology* top, double* msOut);
/* The same through shd_pe_fill_rowstore_shards: a sharded in-process engine
 * needs no gather first.  info (optional) as there. */
int shd_topology_fill_shards(ShdTopology* top, int64_t needBudgetBytes, ShdPeFillShardsInfo* info);
/* ABI 14.  The teardown call: the load of every cached entry with
 * packetCount > 0 (what _topology_logAllCachedPaths logs, joined with the
 * paths), in the stored direction (s, d):
 *  - s == d: the count is added to vertexLoad[s];
 *  - a direct entry: to both end vertices and to the arc s -> d, on the host;
 *  - every other entry is a request (s, d, packetCount) of one
 *    shd_pe_path_load call; one that comes back with a status is skipped and
 *    counted in totals[3] (as is a direct entry whose pair has no arc, which
 *    the cache does not store today).
 * totals[0..2] count the entries, weighted vertices and weighted hops of all
 * three kinds; out->status is not written (the requests are the call's own).
 * The cache stores an undirected pair once, so the packets of both directions
 * are attributed along the stored direction's path: a link's total is the sum
 * of its two arcs.  Not safe against concurrent inserts (shd_rowstore_foreach
 * is not).  top or out NULL: SHD_PE_EINVAL. */
int shd_topology_link_load(ShdTopology* top, const ShdPeLoadOut* out);

/* ------------------------------------------------------------------------
 * GraphML ingestion (host only, no GPU work).  Replaces
 * igraph_read_graph_graphml in _topology_loadGraph (topology.c:371-399) plus
 * the attribute reads the path needs: edge 'latency' (EANV,
 * _topology_extractEdgeWeights topology.c:1212-1246), edge / vertex
 * 'packetloss' (topology.c:402-444, :1442-1462) and the graph string
 * 'preferdirectpaths' (topology.c:769-790, case-insensitive prefix
 * true/yes/1).  `buf` is the (decompressed) GraphML text.  Vertex ids follow
 * <node> order and edge ids <edge> order, as igraph assigns them; a missing or
 * unparsable number is NaN.  Duplicate node ids or an edge naming an unknown
 * node -> SHD_PE_EINVAL. */
typedef struct ShdGraphml ShdGraphml;
int shd_graphml_parse(const char* buf, int64_t len, ShdGraphml** out);
/* Fill a ShdPeGraphDesc whose arrays point into `g` (valid until
 * shd_graphml_free); vertexPacketLoss is NULL when no node 'packetloss' key
 * exists.  Pass it straight to shd_pe_create. */
int shd_graphml_describe(const ShdGraphml* g, ShdPeGraphDesc* desc, int32_t* prefersDirectPaths);
/* The GraphML id string of vertex v (NULL if out of range). */
const char* shd_graphml_vertex_id(const ShdGraphml* g, int32_t v);
void shd_graphml_free(ShdGraphml* g);

/* The vertex attributes topology_attach reads (topology.c:2094-2430), kept by
 * shd_graphml_parse: keys are matched by exact attr.name as
 * igraph_cattribute_has_attr does (_topology_findVertexAttributeString /
 * Double, topology.c:308-347); <default> handling as for the other node keys. */
#define SHD_PE_VATTR_IP          0
#define SHD_PE_VATTR_CITYCODE    1
#define SHD_PE_VATTR_COUNTRYCODE 2
#define SHD_PE_VATTR_GEOCODE     3
#define SHD_PE_VATTR_TYPE        4
#define SHD_PE_VATTR_COUNT       5
typedef struct ShdPeVertexAttrs {
    int32_t nVertices;
    const uint32_t* ip;          /* address_stringToIP(ipStr) (address.c:145-152): inet_pton's s_addr as
                                    the host reads it; 0xffffffff (INADDR_NONE) when the attribute is
                                    absent, empty or unparsable.  NULL = graph has no 'ip' key */
    const int32_t *citycode, *countrycode, *geocode, *type;
                                 /* interned codes >= 0; -1 = absent or empty string
                                    (topology.c:316); NULL = no such key */
    const double *bandwidthDown, *bandwidthUp;   /* NaN = absent; NULL = no key */
} ShdPeVertexAttrs;
/* The arrays live in g (valid until shd_graphml_free). */
int shd_graphml_vertex_attrs(const ShdGraphml* g, ShdPeVertexAttrs* out);
/* A host's hint string in the code space of attribute `attr` (SHD_PE_VATTR_*):
 * two strings share a code iff g_ascii_strcasecmp returns 0 (only ASCII A-Z
 * fold; topology.c:2117-2120).  NULL -> -1 (no hint); an empty string or one
 * no vertex carries -> -2 (a hint that matches nothing); else the code. */
int32_t shd_graphml_attr_code(const ShdGraphml* g, int32_t attr, const char* value);
/* The raw attribute string of vertex v, NULL where
 * _topology_findVertexAttributeString finds none (absent or empty): what the
 * attach message() prints (topology.c:2411-2429). */
const char* shd_graphml_vertex_attr_string(const ShdGraphml* g, int32_t v, int32_t attr);

/* ------------------------------------------------------------------------
 * Host attachment (topology_attach -> _topology_findAttachmentVertex,
 * topology.c:2094-2430): which vertex a host with the given hints lands on.
 * shd_pe_attach_hosts answers `count` hosts at once on the device (attaches do
 * not depend on each other: each host draws from its own Random, host.c:
 * 176-181); shd_pe_attach_host is the same rule for one host on the CPU (an
 * attach after start-up).  Both give identical integers.  The handle is its
 * own object: attach runs before shd_pe_create has its attached[] list.
 *
 * The rule, with usable(x) = x not in {INADDR_NONE 0xffffffff, INADDR_ANY 0,
 * INADDR_LOOPBACK 0x7f000001} compared against the raw s_addr as :2127 and
 * :2264 do (on a little-endian host that keeps 127.0.0.1 = 0x0100007f usable
 * and excludes 1.0.0.127), reqUsable = ipHintGiven && usable(ipHint) and
 * requestedIP = reqUsable ? ipHint : 0 (the helper is g_new0'd, :2255-2268):
 *  - exact IP (:2134-2159): if reqUsable and some vertex has usable(vip) &&
 *    vip == requestedIP, the candidates are exactly those vertices and the
 *    choice is the random one (:2324); candidateSet 8.
 *  - otherwise a vertex matches city when code[v] >= 0 && hint >= 0 &&
 *    code[v] == hint (likewise country, geo, type; :2117-2120), and the first
 *    non-empty set in the order of :2293-2317 is used: 0 city+type, 1 city,
 *    2 country+type, 3 country, 4 geo+type, 5 geo, 6 type, 7 all vertices.
 *  - longest prefix (:2295-2316) applies to sets 0-6 iff reqUsable and the set
 *    holds a usable vertex address, to set 7 iff ipHintGiven and it does (a
 *    given but unusable hint then matches against 0).  _topology_
 *    getLongestPrefixMatch (:2219-2246): match = ~(vip ^ requestedIP) with the
 *    raw vip of every candidate; the first candidate in vertex order with the
 *    maximum match wins, except that a maximum of 0 gives the LAST candidate
 *    (`|| bestMatch == 0` lets every zero replace the previous one).
 *  - random (:2327-2333): the candidate at ordinal
 *    (gint) round((gdouble)((numCandidates - 1) * randomDouble)) in vertex
 *    order (= vertex index order, _topology_iterateAllVertices :980-1017).
 * randomDouble is what random_nextDouble WOULD return for the host; the
 * reference only draws on the random branch, so usedRandom tells the caller
 * whether to advance the host's real Random. */
typedef struct ShdPeAttachHints {            /* `count` hosts, SoA */
    int64_t count;
    const uint8_t*  ipHintGiven;    /* ipHint != NULL */
    const uint32_t* ipHint;         /* address_stringToIP(ipHint), raw */
    const int32_t *citycode, *countrycode, *geocode, *type;   /* -1 none, -2 matches nothing, else code */
    const double*   randomDouble;   /* the value random_nextDouble WOULD return for this host, in [0,1] */
} ShdPeAttachHints;
typedef struct ShdPeAttachResult {           /* any pointer but vertex may be NULL */
    int32_t* vertex;
    uint8_t* candidateSet;          /* 0 city+type, 1 city, 2 country+type, 3 country, 4 geo+type,
                                       5 geo, 6 type, 7 all, 8 exact-IP matches */
    int32_t* numCandidates;
    uint8_t* usedRandom;            /* 1: the reference consumed the draw (:2327); 0: longest prefix */
    uint64_t *bwDown, *bwUp;        /* (guint64) of the chosen vertex's bandwidth (:2398-2409), 0 if NaN
                                       or the graph has no such key */
} ShdPeAttachResult;

typedef struct ShdPeAttach ShdPeAttach;
/* Uploads the vertex table (20 B per vertex) to `device`; va is only borrowed.
 * nVertices <= 0 -> SHD_PE_EINVAL, no gfx950 device -> SHD_PE_ENODEV. */
int shd_pe_attach_new(const ShdPeVertexAttrs* va, int32_t device, ShdPeAttach** out);
void shd_pe_attach_free(ShdPeAttach* at);
/* _topology_findAttachmentVertex for h->count hosts on the device (hosts are
 * staged in chunks; one wave serves a small group of hosts and walks the
 * vertex table in vertex order, so no result depends on scheduling).  A
 * randomDouble outside [0,1] or NaN -> SHD_PE_EINVAL before any work. */
int shd_pe_attach_hosts(ShdPeAttach* at, const ShdPeAttachHints* h, const ShdPeAttachResult* r);
/* Hosts per staging chunk (default 65,536; tests and memory-tight callers). */
int shd_pe_attach_set_chunk(ShdPeAttach* at, int64_t hostsPerChunk);
/* Of the last shd_pe_attach_hosts call: ms[0] device time of its kernels
 * (events), ms[1] wall time of the whole call, staging included. */
int shd_pe_attach_timing(const ShdPeAttach* at, double* ms);
/* The same rule for host i of h on the CPU, one serial pass over the
 * vertices, no GPU (the late single attach, topology.c:2371-2430). */
int shd_pe_attach_host(const ShdPeVertexAttrs* va, const ShdPeAttachHints* h, int64_t i,
                       const ShdPeAttachResult* r);

/* ------------------------------------------------------------------------
 * Graph property check (_topology_checkGraphProperties, topology.c:724-809):
 * igraph_is_connected(IGRAPH_STRONG) (:738), igraph_clusters(IGRAPH_STRONG)
 * (:745) and _topology_isComplete (:754, body :450-552) in one call, before
 * any host attaches and before shd_pe_create: no handle, the call owns its
 * memory.  The reference refuses a graph unless isConnected && clusterCount
 * == 1 (:800-806); that decision stays with the caller.
 *
 * Only nVertices, nEdges, directed, edgeFrom and edgeTo are read; the latency
 * and loss pointers may be NULL (edge values are _topology_checkGraphEdges'
 * job, which shd_pe_create does).
 *
 * Clusters as in igraph 0.7.1: strongly connected components of a directed
 * graph, weak components of an undirected one (igraph ignores the mode there);
 * self-loops and parallel edges are accepted and change nothing; isConnected
 * == (clusterCount == 1) for every n >= 1.  membership (optional, nVertices
 * entries): membership[v] = the smallest vertex id in v's cluster, whatever
 * the schedule.  Completeness: per vertex the OUT-incident edge count,
 * parallel edges each (directed: edges with from == v, a self-loop once;
 * undirected: both endpoints, a self-loop twice, minus one iff v has at least
 * one self-loop); complete iff every count >= nVertices.  isComplete equals
 * shd_pe_is_complete of an engine created from the same description.
 *
 * nVertices <= 0, a NULL out or an endpoint outside [0, nVertices):
 * SHD_PE_EINVAL; 2 * nEdges > INT32_MAX: SHD_PE_ETOOBIG (int32 counts). */
typedef struct ShdPeGraphProps {
    int32_t isDirected;      /* g->directed != 0 */
    int32_t isConnected;     /* igraph_is_connected(IGRAPH_STRONG), topology.c:738 */
    int32_t clusterCount;    /* igraph_clusters(IGRAPH_STRONG) count, :745 */
    int32_t largestCluster;  /* vertices in the largest cluster (no reference counterpart) */
    int32_t isComplete;      /* _topology_isComplete, :450-552 */
    int32_t firstIncomplete; /* the vertex :523-526 reports: lowest v with count < n; -1 if complete */
} ShdPeGraphProps;
typedef struct ShdPeGraphPropsInfo {   /* optional, device call only */
    int64_t sweeps;          /* edge sweeps launched (the counting sweep included) */
    int64_t rounds;          /* decomposition rounds (trim / pivot / colouring; undirected: hook + jump) */
    int32_t handedOff;       /* 1: sweep budget exhausted, answer computed by the host form */
    int64_t usDevice, usCall;/* device events (up to the hand-off, if any); wall time incl. upload */
} ShdPeGraphPropsInfo;
/* On the CPU, one thread: a counting pass, union-find (undirected) or an
 * iterative Tarjan over its own CSR (directed; no recursion). */
int shd_pe_graph_props_host(const ShdPeGraphDesc* g, ShdPeGraphProps* out, int32_t* membership);
/* On gfx950 device `device`: the edge list is uploaded as given (pageable
 * arrays in chunks through page-locked staging) and every kernel is edge- or
 * vertex-parallel; no CSR is built on either side.  sweepBudget <= 0 selects
 * the default; when the edge sweeps of a call reach the budget the whole
 * answer comes from shd_pe_graph_props_host and info->handedOff is 1 (same
 * result by construction).  No gfx950 device: SHD_PE_ENODEV, never a silent
 * host run. */
int shd_pe_graph_props(const ShdPeGraphDesc* g, int32_t device, int32_t sweepBudget,
                       ShdPeGraphProps* out, int32_t* membership, ShdPeGraphPropsInfo* info);

#ifdef __cplusplus
}
#endif
#endif
