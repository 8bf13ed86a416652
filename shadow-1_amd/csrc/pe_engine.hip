// pe_engine.hip -- C-ABI implementation of the MI355X Shadow path engine.
//
// Replaces topology.c:1681-1866 (target collection + igraph Dijkstra +
// per-target fold) with device kernels; see include/shd_pathengine.h.
// No CPU compute fallback: every row comes from a gfx950 kernel, and create
// fails with SHD_PE_ENODEV when no device is usable.
//
// Multi-GPU: the T table rows are split into G contiguous
// row shards of (near-)equal kernel work units (shd_pe_plan_shards).  One
// engine owns one or more of them, one per device (nDevices); several
// engines in several processes own the rest (shardIndex / shardCount).  Each
// shard holds its own graph copy, stream and a shard-sized table
// (rows x T); compute runs all local shards concurrently (one host thread
// per device), never exchanging data.  Reading, copying and exchanging the
// finished rows is pe_rows.hip: there shd_pe_gather assembles the whole
// table on every device with RCCL (a group of broadcasts = all-gather with
// per-shard sizes) over xGMI, or with device copies when several logical
// shards share a device.  The reference serialises every row on one core
// under graphLock (topology.c:1747-1781).
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <chrono>
#include <thread>
#include <vector>

#include "pe_build.hpp"
#include "pe_engine.hpp"
#include "pe_plan.hpp"

using namespace shdpe;

constexpr int LDS_BYTES = 160 * 1024;

template <class T, class A>
static int dev_upload(Shard* s, T** dst, const std::vector<T, A>& src) {
    int rc = dev_alloc(s, dst, src.size());
    if (rc) return rc;
    if (!src.empty())
        HIPCHK(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return SHD_PE_OK;
}

// ... into a member of DevGraph (pointers to const)
template <class T, class A>
static int dev_upload(Shard* s, const T** dst, const std::vector<T, A>& src) {
    T* p = nullptr;
    const int rc = dev_upload(s, &p, src);
    *dst = p;
    return rc;
}

// SHDPE_* tuning variables are read only under SHD_PE_DEBUG_ENV: a library
// linked into Shadow must not change behaviour with the environment.
static void read_tuning(Tuning& t, int32_t flags) {
    if (flags & SHD_PE_DEBUG_COUNTERS) t.debug = 1;
    if (!(flags & SHD_PE_DEBUG_ENV)) return;
    auto gi = [](const char* k, int& v) { const char* e = std::getenv(k); if (e && *e) v = std::atoi(e); };
    auto gd = [](const char* k, double& v) { const char* e = std::getenv(k); if (e && *e) v = std::atof(e); };
    gi("SHDPE_THREADS", t.spThreads);
    gi("SHDPE_HEAVY_DEG", t.heavyDeg);
    gi("SHDPE_LAYOUT", t.layout);
    gi("SHDPE_WG_PER_CU", t.wgPerCU);
    gi("SHDPE_KFLAGS", t.kflags);
    gd("SHDPE_DELTA_FACTOR", t.deltaFactor);
    gi("SHDPE_EXACT_HC", t.exactHc);
    gi("SHDPE_EXACT_PER_CU", t.exactPerCU);
    gi("SHDPE_BATCH", t.batch);
    gi("SHDPE_BATCH_LB", t.batchLB);
    gi("SHDPE_BATCH_GRID", t.batchGrid);
    gi("SHDPE_BATCH_ORDER", t.batchOrder);
    gi("SHDPE_BATCH_WPE", t.batchWpe);
    gi("SHDPE_RELABEL", t.relabel);
    gi("SHDPE_BATCH_SPLIT", t.batchSplit);
    gd("SHDPE_BATCH_DELTA_FACTOR", t.batchDeltaFactor);
    gd("SHDPE_BATCH_SCRATCH_GB", t.batchScratchGB);
    gd("SHDPE_DENSE_MIN", t.denseMin);
    gd("SHDPE_DENSE_BATCH_GB", t.denseBatchGB);
    gi("SHDPE_PRED_MI", t.densePredMi);
    gi("SHDPE_DENSE_EPOCHS", t.denseEpochs);
    gi("SHDPE_DEBUG", t.debug);
    gi("SHDPE_STREAM_WG_PER_CU", t.streamWgPerCU);
    gi("SHDPE_TIE_CORRUPT", t.tieCorrupt);
    gi("SHDPE_PRED_FILTER", t.predFilter);
    gi("SHDPE_POST_SPLIT", t.postSplit);
    gi("SHDPE_LANE_OFFSET", t.laneOffset);
    gi("SHDPE_TUNE_FAIL_WPE", t.failWpe);
    gi("SHDPE_BATCH_ROUND", t.batchRoundCap);
    gi("SHDPE_TIE_SLOTS", t.tieSlotsCap);
    gi("SHDPE_DEVICE_PLAN", t.devicePlan);
    gi("SHDPE_TUNE_LOG", t.tuneLog);
    gi("SHDPE_PATHS_GROUP", t.pathsGroup);
    gi("SHDPE_PATHS_CHUNK", t.pathsChunk);
    gi("SHDPE_PATHS_FAST", t.pathsFast);
    gi("SHDPE_LOAD_SORT", t.loadSort);
    gi("SHDPE_LOAD_SLOTS", t.loadSlots);
    gi("SHDPE_TLOAD_TREE", t.tloadTree);
    gi("SHDPE_TLOAD_CORRUPT", t.tloadCorrupt);
}

extern "C" void shd_pe_default_options(ShdPeOptions* opt) {
    if (!opt) return;
    std::memset(opt, 0, sizeof(*opt));
    opt->device = 0;
    opt->delta = 0.0;
    opt->storePred = 1;
    opt->forceMode = 0;
    opt->nDevices = 1;
    opt->devices = nullptr;
    opt->shardIndex = 0;
    opt->shardCount = 1;
    opt->debugFlags = 0;
}

extern "C" const char* shd_pe_strerror(int code) {
    switch (code) {
        case SHD_PE_OK: return "ok";
        case SHD_PE_EINVAL: return "invalid argument or graph fails topology checks";
        case SHD_PE_ENOMEM: return "out of memory";
        case SHD_PE_ENODEV: return "no usable gfx950 device";
        case SHD_PE_EUNREACHABLE: return "target unreachable";
        case SHD_PE_ENOSELFLOOP: return "self-loop (s,s) missing";
        case SHD_PE_EMULTI: return "multigraph error (reserved: no longer returned)";
        case SHD_PE_EHIP: return "HIP runtime error";
        case SHD_PE_ENOTATTACHED: return "vertex is not attached";
        case SHD_PE_ENOEDGE: return "no edge between the vertices";
        case SHD_PE_ENOTOWNED: return "row belongs to another engine's shard (gather first)";
        case SHD_PE_ETOOBIG: return "graph exceeds the engine's vertex limit";
        case SHD_PE_ECOMM: return "RCCL communicator error";
        default: return "unknown error";
    }
}

static inline int a16(long x) { return (int)((x + 15) & ~15L); }

// The sparse kernel's LDS layout and grid.  False when no layout can hold the
// graph's per-row LDS state.
static bool configure_sparse(ShdPe* pe, Shard* sh) {
    const HostGraph& g = pe->hg;
    const Tuning& tu = pe->tu;
    const long n = g.n;
    const long nw = (n + 31) / 32;
    const int LDS = LDS_BYTES;
    SparseLaunch c{};
    c.threads = std::min(tu.spThreads, sparse_max_threads());
    c.hcap = 256;
    c.heavyDeg = tu.heavyDeg;
    const int qmin = 2048;
    // LDS bytes per layout (queues are ping-pong pairs; LAYOUT 0/3 keep them in HBM)
    const int pend = a16(4 * nw), hbits = a16(4 * nw);
    const int hq2 = 2 * a16(4 * c.hcap);
    const long need2 = 64 + pend + hbits + hq2 + a16(8 * n) + a16(2 * n) + a16(4 * (n + 1));
    const long need1 = 64 + pend + hbits + hq2 + a16(8 * n);
    const long need3 = 64 + pend + a16(8 * n);
    const long need0 = 64 + pend + hbits;
    int layout = 0;
    long used = need0;
    if (need2 + 8 * qmin <= LDS) { layout = 2; used = need2; }
    else if (need1 + 8 * qmin <= LDS) { layout = 1; used = need1; }
    // LAYOUT 3 keeps only dist + pending bits in LDS: ~1.4x slower per row
    // than LAYOUT 2 (measured, C2) but fits more rows per CU; take it when it
    // at least doubles the resident rows.
    const int maxWgByThreads = 2048 / std::max(c.threads, 64);
    const long wg2 = layout == 2 ? std::min<long>(maxWgByThreads, LDS / (need2 + 8 * qmin)) : 0;
    const long wg3 = std::min<long>(maxWgByThreads, LDS / need3);
    if (need3 <= LDS && wg3 >= 2 * std::max<long>(wg2, 1)) { layout = 3; used = need3; }
    if (tu.layout == 3 && need3 <= LDS) { layout = 3; used = need3; }
    else if (tu.layout == 2 && need2 + 8 * qmin <= LDS) { layout = 2; used = need2; }
    else if (tu.layout == 1 && need1 + 8 * qmin <= LDS) { layout = 1; used = need1; }
    else if (tu.layout == 0) { layout = 0; used = need0; }
    c.layout = layout;
    if (layout == 1 || layout == 2) {
        c.qcap = (int)std::min<long>((LDS - used) / 8, std::max<long>(n, 1024)) & ~3;
        c.ldsBytes = (int)(used + 2 * a16(4 * c.qcap));
    } else {
        c.qcap = (int)((n + 63) & ~63L);
        c.ldsBytes = (int)used;
    }
    const int wgPerCU = std::max(1, std::min<int>({tu.wgPerCU, LDS / std::max(c.ldsBytes, 1),
                                                   2048 / c.threads}));
    c.grid = sh->numCUs * wgPerCU;
    c.delta = pe->opt.delta > 0 ? pe->opt.delta : g.meanArcLatency * tu.deltaFactor;
    if (!(c.delta > 0)) c.delta = 1.0;
    c.kflags = tu.kflags;
    sh->cfg = c;
    return !(layout == 0 && need0 > LDS);
}

// The exact kernels' heap split and grid.
static void configure_exact(ShdPe* pe, Shard* sh) {
    const Tuning& tu = pe->tu;
    const long n = pe->hg.n;
    const int LDS = LDS_BYTES;
    // exact kernels: n <= exact_soa_max_n() keeps heap + index2 wholly in
    // LDS (16 B per vertex, several rows per CU); larger graphs keep the top
    // of the heap in LDS (12 B per entry, up to the whole 160 KB) and the
    // tail in the global slot.
    const bool soa = n <= exact_soa_max_n() && tu.exactHc <= 0;
    const long perWG = soa ? 16L * n + 16 : std::min<long>(LDS, 12L * n + 16);
    // (512 B of the LDS stay free for the kernels' static shared variables;
    // k_exact_rows' preferred-child bits take their share when they fit in
    // half of it -- n <= ~650k)
    const long bitsB = !soa && exact_bits_bytes(n) <= LDS / 2 ? exact_bits_bytes(n) : 0;
    sh->exactHc = (int)std::max<long>(
        1, std::min<long>(n, (std::min<long>(LDS - 512 - bitsB, perWG) - 16) / 12));
    if (tu.exactHc > 0) sh->exactHc = std::min(sh->exactHc, tu.exactHc);   // tests: global heap tail
    const int exPerCU = (int)std::max<long>(1, std::min<long>(8, LDS / perWG));
    sh->exactGrid = sh->numCUs * (tu.exactPerCU > 0 ? tu.exactPerCU : exPerCU);
}

// The batched kernel's variants and the shard's plan of them.  False when
// neither the 4- nor the 8-wave variant fits the LDS.
static bool configure_batch(ShdPe* pe, Shard* sh) {
    const HostGraph& g = pe->hg;
    const Tuning& tu = pe->tu;
    const long n = g.n;
    const int LDS = LDS_BYTES;
    BatchLaunch b{};
    // LB = 16 sources per batch; 8 when a shard has too few rows to give
    // every CU a batch of 16.  C4 per-rank shard times, same box: round 5
    // (4-wave relax, one workgroup per CU; profiles/r05_ab_notes.txt r05w)
    // N=4 (4,096 rows) LB 16 28.8 ms vs LB 8 31.0, N=8 (2,048 rows) LB 8 17.2
    // vs LB 16 25.4; round 4 (two 8-wave workgroups per CU, r04_shard_times)
    // had N=4 at LB 8.  LB 4 (32-B line pieces) stays a SHDPE_BATCH_LB option.  (The
    // relax shared by K workgroups per batch and the post kernel over lane
    // slices are patches under tools/variants/)
    b.lb = tu.batchLB;
    if (b.lb != 4 && b.lb != 8 && b.lb != 16 && b.lb != 32)
        b.lb = ((int64_t)sh->rowCount + 15) / 16 >= (int64_t)sh->numCUs ? 16 : 8;
    // (1024 threads, 768 for the 6-wave variant: compile-time in the kernel)
    b.threads = batch_threads(8);
    // pending bitmaps (2 x n/8 bytes) in LDS while they fit beside the
    // control block, else in each slot's global scratch (gbits, LB 16)
    b.gbits = pe->batched && batch_lds_bytes((int)n, 8, false) > LDS ? 1 : 0;
    if (b.gbits) b.lb = 16;
    // (per part: the post kernel's two parts have their own LDS sizes, so the
    // occupancy -- and with it the grid -- is each part's own)
    auto occupancy = [&](int wpe, int threads, int part) {
        const int lds = batch_lds_bytes((int)n, wpe, b.gbits != 0, part);
        int per = 0;
        if (lds > LDS ||
            hipFuncSetAttribute(batch_kernel_ptr(b.lb, wpe, b.gbits != 0, part),
                                hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess ||
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, batch_kernel_ptr(b.lb, wpe, b.gbits != 0, part),
                                                         threads, lds) != hipSuccess)
            per = 0;
        return per;
    };
    // Two kernel variants: 8 waves per SIMD (two 1024-thread workgroups per
    // CU, one vertex per group) and 4 (one workgroup per CU, two vertices
    // per group).  Which is faster differed from box to box of the same SKU
    // in rounds 3-4 (C4 same-box pairs: 172 vs 185 ms on some, 182 vs 142 ms
    // on others; profiles/r03_ab_notes.txt), so shd_pe_tune times them all;
    // SHDPE_BATCH_WPE forces one.  Since the round-5 loops the tune has
    // picked the 4-wave relax on every box (and the 6-wave post kernel for
    // batches of 16, the 4-wave one for 8), so an untuned engine -- the
    // drop-in computes once -- starts there.
    auto make = [&](int wpe, int part = 0) {
        BatchLaunch c = b;
        c.wpe = wpe;
        if (wpe == 6) c.threads = batch_threads(6);   // two 768-thread workgroups per CU
        c.ldsBytes = batch_lds_bytes((int)n, wpe, b.gbits != 0, part);
        const int per = c.ldsBytes <= LDS ? occupancy(wpe, c.threads, part) : 0;
        c.grid = sh->numCUs * std::max(per, 1);
        if (tu.batchGrid > 0 && tu.batchGrid < c.grid) c.grid = tu.batchGrid;
        c.delta = pe->opt.delta > 0 ? pe->opt.delta : g.meanArcLatency * tu.batchDeltaFactor;
        if (!(c.delta > 0)) c.delta = 1.0;
        return std::make_pair(c, per);
    };
    const int forced = tu.batchWpe == 4 || tu.batchWpe == 6 || tu.batchWpe == 8 ? tu.batchWpe : 0;
    auto v8 = make(8), v4 = make(4), v6 = make(6);
    const bool ok8 = v8.second >= 1, ok4 = v4.second >= 1, ok6 = v6.second >= 2 && b.threads == 1024;
    const int first = forced == 6 && ok6 ? 6 : forced == 8 && ok8 ? 8 : ok4 ? 4 : 8;
    v8.first.split = v4.first.split = v6.first.split = tu.batchSplit ? 1 : 0;
    b = first == 8 ? v8.first : first == 6 ? v6.first : v4.first;
    BatchPlan& p = sh->plan;
    p = BatchPlan{};
    p.cand[p.nc++] = b;
    if (!forced && ok8 && ok4) p.cand[p.nc++] = first == 8 ? v4.first : v8.first;
    // the 6-wave variant (768 threads: 80 VGPRs, fewer spills than 8 waves'
    // 64) joins the tune when two of its workgroups fit a CU
    if (!forced && ok6 && tu.batchSplit) p.cand[p.nc++] = v6.first;
    p.relax = p.post = b;
    if (!forced && first == 4 && ok6 && b.split && b.lb >= 16) p.post = v6.first;
    // the post kernel in two parts (PART 5 / 6): every candidate as either
    // part, with the part's own LDS and grid.  An untuned engine runs the one
    // post kernel: the two parts are shd_pe_tune's choice, timed against it on
    // the shard's own rows (measured at C4 only: DESIGN §7), or forced with
    // SHDPE_POST_SPLIT=1 -- then the predecessor part runs the post pick's
    // variant and the label part what the tune picked at C4; ensure_batch
    // drops the split when the per-batch label arrays do not fit.
    // (partsOk: every part of every candidate can be launched -- the
    // occupancy query accepts its LDS size; else the one post kernel stays)
    p.partsOk = true;
    for (int k = 0; k < p.nc; ++k) {
        const auto pr = make(p.cand[k].wpe, 5), lb = make(p.cand[k].wpe, 6);
        p.candPred[k] = pr.first;
        p.candLabel[k] = lb.first;
        p.candPred[k].split = p.candLabel[k].split = p.cand[k].split;
        p.partsOk = p.partsOk && pr.second >= 1 && lb.second >= 1;
    }
    p.redo = p.post;
    p.postSplit = b.split && tu.postSplit == 1 && p.partsOk;
    if (p.postSplit) {
        // (C4's tune, profiles/post_split_phase_cycles_head.txt: the 6-wave
        // predecessor part 17.0 ms against 18.9 / 22.7 at 4 / 8 waves, the 8-wave
        // label part 11.0 ms against 14.4 / 11.5 at 4 / 6)
        const int wpe = p.post.wpe;
        p.post = make(wpe, 5).first;
        p.label = make(!forced && wpe == 6 && ok8 ? 8 : wpe, 6).first;
        p.post.split = p.label.split = 1;
    }
    return ok8 || ok4;
}

// The stats that name the plan's picks (configure, and shd_pe_tune after it
// changed them).
static void plan_stats(const ShdPe* pe, Shard* sh) {
    const BatchPlan& p = sh->plan;
    sh->stats.deltaUsed = pe->batched ? p.relax.delta : sh->cfg.delta;
    sh->stats.batched = pe->batched ? 1 : 0;
    sh->stats.batchLanes = pe->batched ? p.relax.lb : 0;
    sh->stats.batchWaves = pe->batched ? p.relax.wpe : 0;
    sh->stats.batchPostWaves = pe->batched && p.relax.split ? p.post.wpe : 0;
}

// Kernel configuration for one shard's device.  Returns SHD_PE_ETOOBIG when
// no kernel layout can hold the graph's per-row LDS state.
static int configure(ShdPe* pe, Shard* sh) {
    const Tuning& tu = pe->tu;
    const bool sparseFits = configure_sparse(pe, sh);
    configure_exact(pe, sh);
    // Batched multi-source kernel: the layout for graphs whose per-row state
    // does not fit LDS (LAYOUT 0), or on request (forceMode 5).
    pe->batched = pe->mode == 1 &&
                  (tu.batch == 1 || (tu.batch != 0 && sh->cfg.layout == 0) || pe->opt.forceMode == 5);
    const bool batchFits = configure_batch(pe, sh);
    if (pe->batched && !batchFits) return SHD_PE_ETOOBIG;
    if (!pe->batched && !sparseFits) return SHD_PE_ETOOBIG;
    plan_stats(pe, sh);
    return SHD_PE_OK;
}

static void destroy_shard(Shard* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    if (s->comm) (void)ncclCommDestroy(s->comm);
    for (void* p : s->allocs) (void)hipFree(p);
    if (s->bsc.LB) (void)hipFree(s->bsc.LB);
    if (s->bsc.redo) (void)hipFree(s->bsc.redo);
    if (s->dPosOf) (void)hipFree(s->dPosOf);
    for (hipEvent_t e : {s->ev0, s->ev1, s->evA, s->evB, s->evP[0], s->evP[1], s->evP[2], s->evP[3]})
        if (e) (void)hipEventDestroy(e);
    if (s->stream) (void)hipStreamDestroy(s->stream);
    if (s->copyStream) (void)hipStreamDestroy(s->copyStream);
}

// Upload `g` as a DevGraph; `attached` is in g's vertex ids.  oldOf == null:
// g is the caller's graph.  Otherwise g = relabel_graph(caller's, *oldOf),
// device id k being the caller's vertex oldOf[k]; kernels map pred back
// through DevGraph::oldId.
static int upload_graph(const HostGraph& g, const std::vector<int32_t>& attached,
                        const std::vector<int32_t>* oldOf, Shard* sh, DevGraph* out) {
    const int32_t n = g.n;
    DevGraph d{};
    d.n = n;
    d.T = (int32_t)attached.size();
    int rc = SHD_PE_OK;
    // (after a failure the rest are skipped)
    auto up = [&](auto& member, const auto& v) { if (!rc) rc = dev_upload(sh, &member, v); };
    std::vector<uint8_t> isAtt(n, 0);
    for (int32_t v : attached) isAtt[v] = 1;
    up(d.rowPtr, g.rowPtr); up(d.col, g.col); up(d.lat, g.lat); up(d.rel, g.rel);
    up(d.outToIn, g.outToIn);
    up(d.vrel, g.vrel); up(d.selfLat, g.selfLat); up(d.selfRel, g.selfRel);
    up(d.selfMinLat, g.selfMinLat); up(d.selfMinRel, g.selfMinRel); up(d.hasSelf, g.hasSelf);
    up(d.attached, attached); up(d.isAttached, isAtt);
    {
        std::vector<Arc> arcs(g.col.size());
        // (pad = the arc's slot in its head's in-list: the batched relax flags
        // that slot for the predecessor filter without a second load)
        for (size_t a = 0; a < arcs.size(); ++a) arcs[a] = Arc{g.lat[a], g.col[a], g.outToIn[a]};
        up(d.arcs, arcs);
        std::vector<Arc3> a3(g.col.size());
        for (size_t a = 0; a < a3.size(); ++a) {
            uint64_t bits;
            std::memcpy(&bits, &g.lat[a], 8);
            a3[a] = Arc3{g.col[a], (uint32_t)bits, (uint32_t)(bits >> 32)};
        }
        up(d.arc3, a3);
    }
    {
        const int hd = sh->cfg.heavyDeg;
        std::vector<uint32_t> hb((n + 31) / 32, 0u);
        for (int32_t v = 0; v < n; ++v)
            if (g.rowPtr[v + 1] - g.rowPtr[v] >= hd) hb[v >> 5] |= 1u << (v & 31);
        up(d.heavyBits, hb);
    }
    if (g.directed) {
        up(d.inPtr, g.inPtr); up(d.inCol, g.inCol); up(d.inLat, g.inLat); up(d.inRel, g.inRel);
    } else {
        d.inPtr = d.rowPtr; d.inCol = d.col; d.inLat = d.lat; d.inRel = d.rel;
    }
    if (g.latFold) { up(d.flat, g.foldLat); up(d.srel, g.selfPathRel); }
    if (oldOf) up(d.oldId, *oldOf);
    if (rc) return rc;
    *out = d;
    return SHD_PE_OK;
}

// The batched path's device ids, built once per create: the caller's graph
// relabelled by descending degree (stable) -- a wave's groups get vertices of
// similar degree in the queue and predecessor pass (less divergence), and the
// hubs' [v][LB] lines sit together -- with the attached list in those ids.
struct Relabelled {
    std::vector<int32_t> oldOf, attached;
    HostGraph g;
};

// Select the shard's device; it must be a gfx950.
static int open_device(Shard* sh) {
    if (hipSetDevice(sh->device) != hipSuccess) return SHD_PE_ENODEV;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, sh->device) != hipSuccess) return SHD_PE_ENODEV;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return SHD_PE_ENODEV;
    sh->numCUs = prop.multiProcessorCount;
    return SHD_PE_OK;
}

// Device state of one shard: graph upload, stream, events, kernel config.
// `rl` (null: none) is what the path kernels get instead of the caller's ids.
// `built` (null: none) is the device build's graph: the first shard on its
// device adopts the arrays as its dgAux instead of uploading HostGraph.
static int init_shard(ShdPe* pe, Shard* sh, const Relabelled* rl, BuiltGraph* built) {
    const HostGraph& g = pe->hg;
    int rc = open_device(sh);
    if (rc) return rc;
    if (hipStreamCreateWithFlags(&sh->stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&sh->copyStream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&sh->ev0) != hipSuccess || hipEventCreate(&sh->ev1) != hipSuccess ||
        hipEventCreate(&sh->evA) != hipSuccess || hipEventCreate(&sh->evB) != hipSuccess ||
        hipEventCreate(&sh->evP[0]) != hipSuccess || hipEventCreate(&sh->evP[1]) != hipSuccess ||
        hipEventCreate(&sh->evP[2]) != hipSuccess || hipEventCreate(&sh->evP[3]) != hipSuccess)
        return SHD_PE_ENODEV;
    if ((rc = configure(pe, sh))) return rc;
    if (built && !built->adopted && !built->allocs.empty() && built->device == sh->device) {
        sh->allocs.insert(sh->allocs.end(), built->allocs.begin(), built->allocs.end());
        built->adopted = true;
        sh->dgAux = built->dg;
        if ((rc = finish_built_graph(pe->attached, sh->cfg.heavyDeg, sh->stream, &sh->dgAux, &sh->allocs)))
            return rc;
    } else if ((rc = upload_graph(g, pe->attached, nullptr, sh, &sh->dgAux))) {
        return rc;
    }
    sh->dg = sh->dgAux;
    if (rl && (rc = upload_graph(rl->g, rl->attached, &rl->oldOf, sh, &sh->dg))) return rc;
    sh->stats.mode = pe->mode;
    sh->stats.isComplete = g.isComplete ? 1 : 0;
    sh->stats.nVertices = g.n;
    sh->stats.nArcs = g.nArcs();
    sh->stats.nAttached = (int32_t)pe->attached.size();
    return SHD_PE_OK;
}

// The HIP ordinals of the engine's shards, each in range.
static int resolve_devices(const ShdPeOptions& o, std::vector<int>& devs) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return SHD_PE_ENODEV;
    devs.resize(o.nDevices);
    for (int i = 0; i < o.nDevices; ++i) {
        devs[i] = o.devices ? o.devices[i] : o.device + i;
        if (devs[i] < 0 || devs[i] >= ndev) return SHD_PE_ENODEV;
    }
    return SHD_PE_OK;
}

static double wall_ms(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// The engine's graph by the device build on the first shard's device, or by
// the host form where the device build hands off.
static int build_graph_on_device(const ShdPeGraphDesc* graph, const ShdPeOptions& o, const std::vector<int>& devs,
                                 HostGraph* hg, BuiltGraph* built, ShdPeBuildInfo* info) {
    Shard probe;
    probe.device = devs[0];
    int rc = open_device(&probe);
    if (rc) return rc;
    int32_t maxN = BUILD_MAX_N;
    if (o.debugFlags & SHD_PE_DEBUG_ENV) {
        const char* e = std::getenv("SHDPE_BUILD_MAXN");
        if (e && *e && std::atoi(e) > 0) maxN = std::min(maxN, (int32_t)std::atoi(e));
    }
    if ((rc = device_build_graph(graph, devs[0], maxN, hg, built, info))) return rc;
    info->built = info->handedOff ? SHD_PE_BUILD_HOST : SHD_PE_BUILD_DEVICE;
    if (!info->handedOff) return SHD_PE_OK;
    built->release();                    // device memory released before the host run
    *hg = HostGraph{};
    const auto t0 = std::chrono::steady_clock::now();
    rc = build_host_graph(graph, hg);
    info->msHostBuild = wall_ms(t0);
    return rc;
}

static int upload_plan_inputs(ShdPe* pe, Shard* sh);

// Create, both entry points: everything after the graph exists is shared.
static int create_engine(const ShdPeGraphDesc* graph, const int32_t* attached, int32_t nAttached,
                         const ShdPeOptions* opt, int32_t graphBuild, ShdPeBuildInfo* infoOut, ShdPe** out) {
    if (graphBuild != SHD_PE_BUILD_HOST && graphBuild != SHD_PE_BUILD_DEVICE && graphBuild != SHD_PE_BUILD_AUTO)
        return SHD_PE_EINVAL;
    ShdPeBuildInfo info;
    std::memset(&info, 0, sizeof(info));
    if (infoOut) *infoOut = info;
    if (!out || !graph || nAttached <= 0 || !attached) return SHD_PE_EINVAL;
    *out = nullptr;
    const auto tCreate = std::chrono::steady_clock::now();
    std::unique_ptr<ShdPe> pe(new (std::nothrow) ShdPe());
    if (!pe) return SHD_PE_ENOMEM;
    if (opt) pe->opt = *opt; else shd_pe_default_options(&pe->opt);
    ShdPeOptions& o = pe->opt;
    if (o.nDevices <= 0) o.nDevices = 1;
    if (o.shardCount <= 0) o.shardCount = 1;
    if (o.shardIndex < 0 || o.shardIndex >= o.shardCount || o.nDevices > 64) return SHD_PE_EINVAL;
    read_tuning(pe->tu, o.debugFlags);
    const bool onDevice = graphBuild == SHD_PE_BUILD_DEVICE ||
                          (graphBuild == SHD_PE_BUILD_AUTO && graph->nEdges >= BUILD_AUTO_MIN_EDGES);
    std::vector<int> devs;
    BuiltGraph built;                    // declared before the shards' uploads: what no shard adopts is freed on return
    int rc;
    if (onDevice) {
        // the device comes first here: without one there is no build to run
        if ((rc = resolve_devices(o, devs))) return rc;
        rc = build_graph_on_device(graph, o, devs, &pe->hg, &built, &info);
    } else {
        const auto t0 = std::chrono::steady_clock::now();
        rc = build_host_graph(graph, &pe->hg);
        info.built = SHD_PE_BUILD_HOST;
        info.msHostBuild = wall_ms(t0);
    }
    if (infoOut) *infoOut = info;
    if (rc) return rc;
    const HostGraph& g = pe->hg;
    pe->posOf.assign(g.n, -1);
    for (int32_t i = 0; i < nAttached; ++i) {
        const int32_t v = attached[i];
        if (v < 0 || v >= g.n) return SHD_PE_EINVAL;
        if (pe->posOf[v] < 0) {
            pe->posOf[v] = (int32_t)pe->attached.size();
            pe->attached.push_back(v);
        }
    }
    const int32_t T = (int32_t)pe->attached.size();
    // ---- devices ----
    if (devs.empty() && (rc = resolve_devices(o, devs))) return rc;
    pe->mode = select_mode(pe->hg, o.forceMode, pe->tu.denseMin);
    pe->G = o.shardCount * o.nDevices;
    pe->firstShard = o.shardIndex * o.nDevices;
    // the batched-kernel decision (and so the shard unit) needs a configured
    // shard: configure a probe on the first device with the whole table
    {
        Shard probe;
        probe.device = devs[0];
        if ((rc = open_device(&probe))) return rc;
        probe.rowCount = T;
        if ((rc = configure(pe.get(), &probe))) return rc;
    }
    pe->bounds.assign(pe->G + 1, 0);
    (void)shd_pe_plan_shards(T, pe->G, pe->batched ? 16 : 1, pe->bounds.data());
    pe->ownStart = pe->bounds[pe->firstShard];
    pe->ownEnd = pe->bounds[pe->firstShard + o.nDevices];
    Relabelled rl;                       // dropped on return: the shards hold their uploads
    const bool relabel = pe->batched && pe->tu.relabel == 1;
    if (relabel) {
        rl.oldOf = degree_order(g);
        rl.g = relabel_graph(g, rl.oldOf);
        pe->devOf.assign(g.n, 0);
        for (int32_t k = 0; k < g.n; ++k) pe->devOf[rl.oldOf[k]] = k;
        for (int32_t v : pe->attached) rl.attached.push_back(pe->devOf[v]);
    }
    for (int i = 0; i < o.nDevices; ++i) {
        std::unique_ptr<Shard> sh(new (std::nothrow) Shard());
        if (!sh) return SHD_PE_ENOMEM;
        sh->gindex = pe->firstShard + i;
        sh->device = devs[i];
        sh->rowStart = pe->bounds[sh->gindex];
        sh->rowCount = pe->bounds[sh->gindex + 1] - sh->rowStart;
        sh->fullOwner = std::find(devs.begin(), devs.begin() + i, devs[i]) == devs.begin() + i;
        rc = init_shard(pe.get(), sh.get(), relabel ? &rl : nullptr, &built);
        pe->shards.push_back(std::move(sh));
        if (rc) { shd_pe_destroy(pe.release()); return rc; }
    }
    if (pe->mode == 1 && pe->batched) {
        BatchRanks br = batch_ranks(g, pe->attached, pe->posOf, pe->tu.batchOrder);
        pe->rank.swap(br.rank);
        pe->rowOff.swap(br.rowOff);
        pe->hubGroups = std::move(br.groups);
        for (auto& sh : pe->shards)
            if ((rc = upload_plan_inputs(pe.get(), sh.get()))) { shd_pe_destroy(pe.release()); return rc; }
    }
    pe->rowDone.reset(new (std::nothrow) std::atomic<uint8_t>[T]);
    if (!pe->rowDone) { shd_pe_destroy(pe.release()); return SHD_PE_ENOMEM; }
    for (int32_t i = 0; i < T; ++i) pe->rowDone[i].store(0, std::memory_order_relaxed);
    if (infoOut) {
        info.msCreate = wall_ms(tCreate);
        *infoOut = info;
    }
    *out = pe.release();
    return SHD_PE_OK;
}

// The device plan's inputs (DevPlan) of a shard, from the host versions create
// just made; freed with the shard.  Without hub groups (orders 0 and 1) or
// with more groups than a wave has lanes the shard has none and plans on the
// host.
static int upload_plan_inputs(ShdPe* pe, Shard* sh) {
    const HubGroups& hg = pe->hubGroups;
    const size_t T = pe->rank.size();
    if (hg.empty() || hg.G > 64 || T == 0 || pe->rowOff.size() != T || hg.dist.size() != T * (size_t)hg.G)
        return SHD_PE_OK;
    HIPCHK(hipSetDevice(sh->device));
    DevPlan& dp = sh->dplan;
    int rc;
    if ((rc = dev_alloc(sh, &dp.rank, T)) || (rc = dev_alloc(sh, &dp.rowOff, T)) ||
        (rc = dev_alloc(sh, &dp.hubDist, T * (size_t)hg.G)))
        return rc;
    HIPCHK(hipMemcpy(dp.rank, pe->rank.data(), T * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dp.rowOff, pe->rowOff.data(), T * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dp.hubDist, hg.dist.data(), T * (size_t)hg.G * 8, hipMemcpyHostToDevice));
    dp.T = (int32_t)T;
    dp.G = hg.G;
    const double mean = pe->hg.meanArcLatency;
    dp.unit = mean > 0.0 && std::isfinite(mean) ? mean : 1.0;
    return SHD_PE_OK;
}

extern "C" int shd_pe_create(const ShdPeGraphDesc* graph, const int32_t* attached,
                             int32_t nAttached, const ShdPeOptions* opt, ShdPe** out) {
    return create_engine(graph, attached, nAttached, opt, SHD_PE_BUILD_HOST, nullptr, out);
}

extern "C" int shd_pe_create_built(const ShdPeGraphDesc* graph, const int32_t* attached, int32_t nAttached,
                                   const ShdPeOptions* opt, int32_t graphBuild, ShdPeBuildInfo* info,
                                   ShdPe** out) {
    return create_engine(graph, attached, nAttached, opt, graphBuild, info, out);
}

// shd_pe_graph_digest: see the header for the order of the entries.
// (undirected: the IN arrays alias the OUT arrays and digest like them)
static int digest_dev_graph(Shard* sh, const DevGraph& d, int64_t nArcs, bool withOldId, uint64_t* dAcc,
                            uint64_t* out) {
    const int64_t n = d.n, np1 = d.n + 1;
    struct A { const void* p; int w; int64_t c; };
    const A arr[] = {
        {d.rowPtr, 4, np1}, {d.col, 4, nArcs}, {d.lat, 8, nArcs}, {d.arcs, 8, 2 * nArcs}, {d.arc3, 4, 3 * nArcs},
        {d.rel, 8, nArcs}, {d.inPtr, 4, np1}, {d.inCol, 4, nArcs}, {d.inLat, 8, nArcs}, {d.inRel, 8, nArcs},
        {d.outToIn, 4, nArcs}, {d.vrel, 8, n}, {d.selfLat, 8, n}, {d.selfRel, 8, n}, {d.hasSelf, 1, n},
        {d.selfMinLat, 8, n}, {d.selfMinRel, 8, n}, {d.attached, 4, d.T}, {d.isAttached, 1, n},
        {d.heavyBits, 4, (n + 31) / 32}, {d.flat, 8, nArcs}, {d.srel, 8, nArcs}, {d.oldId, 4, n}};
    const int count = withOldId ? 23 : 22;
    for (int i = 0; i < count; ++i) {
        const int rc = device_array_digest(arr[i].p, arr[i].w, arr[i].c, dAcc, sh->stream, &out[i]);
        if (rc) return rc;
    }
    return SHD_PE_OK;
}

extern "C" int shd_pe_graph_digest(ShdPe* pe, int32_t shard, uint64_t* out, int32_t cap, int32_t* count) {
    constexpr int32_t N_ENTRIES = 64;
    if (count) *count = N_ENTRIES;
    if (!pe || !out || shard < 0 || shard >= (int32_t)pe->shards.size() || cap < N_ENTRIES) return SHD_PE_EINVAL;
    std::lock_guard<std::mutex> lock(pe->mu);
    for (int i = 0; i < N_ENTRIES; ++i) out[i] = 0;
    const HostGraph& g = pe->hg;
    auto hd = [&](const auto& v) { return host_array_digest(v.data(), (int)sizeof(v[0]), (int64_t)v.size()); };
    int k = 0;
    out[k++] = hd(g.rowPtr); out[k++] = hd(g.col); out[k++] = hd(g.lat); out[k++] = hd(g.rel);
    out[k++] = hd(g.outToIn); out[k++] = hd(g.inPtr); out[k++] = hd(g.inCol); out[k++] = hd(g.inLat);
    out[k++] = hd(g.inRel); out[k++] = hd(g.foldLat); out[k++] = hd(g.selfPathRel); out[k++] = hd(g.vrel);
    out[k++] = hd(g.selfLat); out[k++] = hd(g.selfRel); out[k++] = hd(g.selfMinLat); out[k++] = hd(g.selfMinRel);
    out[k++] = hd(g.hasSelf); out[k++] = hd(g.edgeCount);
    {
        uint64_t s[7] = {(uint64_t)g.n, (uint64_t)g.directed, (uint64_t)g.nEdges, g.latFold ? 1u : 0u,
                         g.isComplete ? 1u : 0u, 0, 0};
        std::memcpy(&s[5], &g.meanArcLatency, 8);
        std::memcpy(&s[6], &g.minArcLatency, 8);
        out[k++] = host_array_digest(s, 8, 7);
    }
    Shard* sh = pe->shards[shard].get();
    HIPCHK(hipSetDevice(sh->device));
    uint64_t* dAcc = nullptr;
    if (hipMalloc((void**)&dAcc, 8) != hipSuccess) return SHD_PE_ENOMEM;
    int rc = digest_dev_graph(sh, sh->dgAux, g.nArcs(), false, dAcc, &out[k]);
    k += 22;
    if (!rc && sh->dg.rowPtr != sh->dgAux.rowPtr) rc = digest_dev_graph(sh, sh->dg, g.nArcs(), true, dAcc, &out[k]);
    (void)hipFree(dAcc);
    return rc;
}

// The field arrays of a table of `rows` rows at position 0 (pred only with
// storePred); `t` is written once all of them are there.
int shdpe::alloc_table(Shard* sh, DevTable& t, size_t rows, size_t T, bool storePred) {
    DevTable a{};
    a.T = (int64_t)T;
    for (const TableField& f : TABLE_FIELDS) {
        if (f.off == (int32_t)offsetof(DevTable, pred) && !storePred) continue;
        unsigned char* p;
        const int rc = dev_alloc(sh, &p, rows * T * (size_t)f.esize);
        if (rc) return rc;
        set_table_field(a, f, p);
    }
    t = a;
    return SHD_PE_OK;
}

int shdpe::ensure_table(ShdPe* pe, Shard* sh) {
    if (sh->tableReady) return SHD_PE_OK;
    int rc;
    if ((rc = alloc_table(sh, sh->tab, (size_t)sh->rowCount, pe->attached.size(), pe->opt.storePred != 0)))
        return rc;
    sh->tab.rowStart = sh->rowStart;
    // scratch slots
    const size_t slots = (size_t)(pe->batched ? sh->exactGrid : std::max(sh->cfg.grid, sh->exactGrid));
    const size_t stride = ((size_t)pe->hg.n + 63) & ~(size_t)63;
    const size_t heapStride = std::max<size_t>(1, (size_t)pe->hg.n - (size_t)sh->exactHc);
    // (a heap tail entry: an f64 key and, behind the slot's keys, an i32 vertex id in 16 B)
    if ((rc = dev_alloc(sh, &sh->sc.dist, slots * stride)) ||
        (rc = dev_alloc(sh, &sh->sc.hops, slots * stride)) ||
        (rc = dev_alloc(sh, &sh->sc.rel, slots * stride)) ||
        (rc = dev_alloc(sh, &sh->sc.pred, slots * stride)) ||
        (rc = dev_alloc(sh, &sh->sc.heapTail, (size_t)sh->exactGrid * heapStride * 2)) ||
        (rc = dev_alloc(sh, &sh->sc.index2, (size_t)sh->exactGrid * stride)))
        return rc;
    sh->sc.heapStride = (int64_t)heapStride;
    sh->sc.stride = (int64_t)stride;
    sh->sc.lfold = nullptr;
    if (pe->hg.latFold && (rc = dev_alloc(sh, &sh->sc.lfold, slots * stride))) return rc;
    if (!pe->batched && (sh->cfg.layout == 3 || sh->cfg.layout == 0)) {
        const size_t per = 2 * ((size_t)sh->cfg.qcap + sh->cfg.hcap);
        if ((rc = dev_alloc(sh, &sh->sc.queue, (size_t)sh->cfg.grid * per))) return rc;
    }
    sh->rowsCap = (int32_t)std::max<size_t>(1, std::min<size_t>(sh->rowCount, 1 << 20));
    if ((rc = dev_alloc(sh, &sh->dRows, (size_t)sh->rowsCap)) ||
        (rc = dev_alloc(sh, &sh->dRowAmbig, (size_t)sh->rowsCap)))
        return rc;
    if (pe->tu.debug) {          // 64 B of counters per row
        if ((rc = dev_alloc(sh, &sh->dDbg, (size_t)sh->rowsCap * 16)) ||
            (rc = dev_alloc(sh, &sh->dXdbg, (size_t)sh->rowsCap * 8)))
            return rc;
    }
    sh->tableReady = true;
    return SHD_PE_OK;
}

// Tie slots for the early-stop emulation (all three relax paths): D f64 + P i32
// + H i32 + R f64 per vertex, <= 2 GiB, <= 254 slots (rowAmbig stores
// 2 + slot in a byte; mode 3: <= 4096, see below); arc indices carry TIE_AMB
// in bit 30.
static int ensure_tie(ShdPe* pe, Shard* sh) {
    if (sh->dTie || sh->tieTried) return SHD_PE_OK;
    sh->tieTried = true;
    int rc;
    const size_t perTie = (size_t)pe->hg.n * 24;
    // (the dense path, mode 3, keeps slots out of rowAmbig's byte: more of them,
    // so its early-stop tie rows run in one launch)
    size_t cap = std::min<size_t>({pe->mode == 3 ? (size_t)4096 : (size_t)254, (size_t)sh->rowsCap,
                                   ((size_t)2 << 30) / perTie});
    if (pe->hg.nArcs() >= ((int64_t)1 << 30)) cap = 0;
    // tests only (SHDPE_TIE_SLOTS): fewer slots, or none as past 2^30 arcs
    if (pe->tu.tieSlotsCap >= 0) cap = std::min(cap, (size_t)pe->tu.tieSlotsCap);
    if (cap > 0) {
        TieBuf t{}, *dd;
        int32_t *sl, *rq;
        const size_t cn = cap * (size_t)pe->hg.n;
        // (count: 4 words, [0] slot counter, [1] the round word of the deferred export;
        // the batched path's post kernel defers its export to k_tie_export)
        if ((rc = dev_alloc(sh, &t.D, cn)) || (rc = dev_alloc(sh, &t.P, cn)) ||
            (rc = dev_alloc(sh, &t.H, cn)) || (rc = dev_alloc(sh, &t.R, cn)) ||
            (rc = dev_alloc(sh, &t.thr, cap)) || (rc = dev_alloc(sh, &t.count, 4)) ||
            (rc = dev_alloc(sh, &sl, (size_t)sh->rowsCap)) ||
            (rc = dev_alloc(sh, &dd, 1)) || (rc = dev_alloc(sh, &rq, cap * 4)))
            return rc;
        t.cap = (int32_t)cap;
        t.n = (int64_t)pe->hg.n;
        t.req = pe->batched ? rq : nullptr;
        t.round = t.count + 1;
        sh->tie = t;
        sh->dSlots = sl;
        sh->dTie = dd;
        HIPCHK(hipMemcpy(sh->dTie, &sh->tie, sizeof(TieBuf), hipMemcpyHostToDevice));
    }
    return SHD_PE_OK;
}

// Post kernel in two parts: the label records cross from the predecessor part
// to the label part, so they need one array per batch of the round like the
// dist arrays, at 16 B per entry beside the dist arrays' 8 (C4: 26 GB beside
// 13).  Allocated only for a shard that runs the two parts -- shd_pe_tune
// while it times them, and afterwards if it keeps them; SHDPE_POST_SPLIT=1 --
// and only where they fit under the scratch budget (batchScratchGB, 64 GiB)
// with 12 GiB left free for what is allocated later; released when the tune
// keeps the one post kernel.  False: the shard runs the one post kernel (C5:
// its round of 131 GB of dist arrays would need 262 GB of label arrays).
static void release_label_arrays(Shard* sh) {
    if (sh->bsc.LB) (void)hipFree(sh->bsc.LB);
    if (sh->bsc.redo) (void)hipFree(sh->bsc.redo);
    sh->bsc.LB = nullptr;
    sh->bsc.redo = nullptr;
    sh->postSplitOk = false;
}

static bool ensure_label_arrays(ShdPe* pe, Shard* sh) {
    if (sh->postSplitOk) return true;
    const BatchPlan& plan = sh->plan;
    if (!sh->batchReady || !plan.relax.split || !plan.partsOk || pe->tu.postSplit == 0) return false;
    // (the tune's choice, not SHDPE_POST_SPLIT=1: only shards with at least a
    // batch per resident workgroup of the 6- / 8-wave variants.  Below that
    // every kernel is one batch long and a third kernel only adds a tail: the
    // C4 N=8 shard, 256 batches of 8, was 15.3-15.4 ms on the two parts the
    // tune's event times preferred, against 15.1-15.2 ms)
    const size_t nBatchesAll = ((size_t)sh->rowCount + (size_t)plan.relax.lb - 1) / (size_t)plan.relax.lb;
    if (pe->tu.postSplit != 1 && nBatchesAll < 2 * (size_t)sh->numCUs) return false;
    const size_t bytes = (size_t)sh->batchRound * (size_t)sh->bsc.nStride * (size_t)plan.relax.lb * sizeof(BLabel);
    size_t freeB = 0, totalB = 0;
    if (hipMemGetInfo(&freeB, &totalB) != hipSuccess) return false;
    if ((double)bytes > pe->tu.batchScratchGB * (double)(1ull << 30) || freeB < bytes + ((size_t)12 << 30)) return false;
    if (hipMalloc(reinterpret_cast<void**>(&sh->bsc.LB), bytes) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&sh->bsc.redo), ((size_t)sh->batchRound + REDO_LIST) * 4) != hipSuccess) {
        (void)hipGetLastError();
        release_label_arrays(sh);
        return false;
    }
    sh->postSplitOk = true;
    return true;
}

static int ensure_batch(ShdPe* pe, Shard* sh) {
    if (sh->batchReady) return SHD_PE_OK;
    const size_t NS = ((size_t)pe->hg.n + 63) & ~(size_t)63;
    BatchPlan& plan = sh->plan;
    const size_t LB = (size_t)plan.relax.lb;
    const size_t bitBytes = plan.relax.gbits ? (size_t)batch_bits_words(pe->hg.n) * 4 : 0;
    const size_t perSlot = NS * LB * (8 + 16) + NS * 4 + bitBytes;   // D, L
    // scratch budget (default 64 GiB): fewer resident batches on huge graphs
    const double budget = pe->tu.batchScratchGB * (double)(1ull << 30);
    const size_t maxSlots = std::max<size_t>(1, (size_t)(budget / (double)perSlot));
    const size_t nBatchesAll = ((size_t)sh->rowCount + LB - 1) / LB;
    size_t grid = 0;                               // the candidates' largest
    for (int k = 0; k < plan.nc; ++k) grid = std::max(grid, (size_t)plan.cand[k].grid);
    const size_t slots = std::min<size_t>({grid, maxSlots, std::max<size_t>(1, nBatchesAll)});
    // a workgroup indexes its scratch slot by blockIdx: no launch may have
    // more workgroups than slots, so every grid of the plan is lowered here
    sh->batchSlots = (int32_t)slots;
    for (int k = 0; k < plan.nc; ++k) plan.cand[k].grid = std::min(plan.cand[k].grid, sh->batchSlots);
    plan.relax.grid = std::min(plan.relax.grid, sh->batchSlots);
    plan.post.grid = std::min(plan.post.grid, sh->batchSlots);
    plan.label.grid = std::min(plan.label.grid, sh->batchSlots);
    plan.redo.grid = std::min(plan.redo.grid, sh->batchSlots);
    for (int k = 0; k < plan.nc; ++k) {
        plan.candPred[k].grid = std::min(plan.candPred[k].grid, sh->batchSlots);
        plan.candLabel[k].grid = std::min(plan.candLabel[k].grid, sh->batchSlots);
    }
    int rc;
    // split kernels: one persisted dist array per batch of a round (relax ->
    // post), the rest per resident workgroup; rounds sized by free memory
    // (at most 160 GiB of dist arrays: C4 one round of 13 GB, C5 one round
    // of 131 GB beside its 107 GB table -- 2 rounds under a 96 GiB cap were
    // 5% slower, profiles/r04_ab_notes.txt r04i)
    // predecessor filter (split kernels): one flag bit per in-arc slot per
    // batch of the round, counted with the round's dist arrays
    const size_t mStride = ((size_t)pe->hg.nArcs() + 127) & ~(size_t)127;
    const bool filter = plan.relax.split && pe->tu.predFilter != 0 && mStride > 0;
    // the device plan's scratch (its inputs were allocated at create, so the
    // free memory read below is already less by them): budgeted with the
    // per-slot scratch still to allocate
    DevPlan& dp = sh->dplan;
    size_t planBytes = 0;
    if (dp.inputs() && pe->tu.devicePlan != 0) {
        // (sized by the rows alone, like dBatchRows: a trial's lanes need not be the plan's)
        dp.capRows = dp.capBatches = sh->rowsCap;
        // (a failed size query: no scratch, the shard plans on the host as before)
        dp.tempBytes = plan_dev_temp_bytes(dp.capRows, dp.capBatches);
        if (dp.tempBytes)
            planBytes = dp.tempBytes + ((size_t)dp.capRows + 64) * (12 + 12) + (size_t)dp.capBatches * 24;
    }
    size_t roundB = slots;
    if (plan.relax.split) {
        size_t freeB = 0, totalB = 0;
        if (hipMemGetInfo(&freeB, &totalB) != hipSuccess) freeB = (size_t)16 << 30;
        const size_t perD = NS * LB * 8 + (filter ? mStride / 8 : 0);
        const size_t rest = slots * (perSlot - NS * LB * 8) + planBytes;
        // (tests only, SHDPE_BATCH_ROUND: fewer batches per round than would fit)
        roundB = batch_round_size(slots, nBatchesAll, perD, rest, freeB, pe->tu.batchRoundCap);
    }
    sh->batchRound = (int32_t)roundB;
    // (the queues' and the flags' 16 spare words: `next` sits behind the queues)
    if ((rc = dev_alloc(sh, &sh->bsc.D, roundB * NS * LB)) || (rc = dev_alloc(sh, &sh->bsc.L, slots * NS * LB)) ||
        (rc = dev_alloc(sh, &sh->bsc.queue, slots * NS + 16)) ||
        (rc = dev_alloc(sh, &sh->dBatchRows, (size_t)sh->rowsCap + 64)) ||
        (rc = dev_alloc(sh, &sh->dLaneOff, (size_t)sh->rowsCap + 64)) ||
        (rc = dev_alloc(sh, &sh->dBatchAmb, (size_t)sh->rowsCap + 64)) ||
        (rc = dev_alloc(sh, &sh->bsc.flags, roundB + 16)))
        return rc;
    if (planBytes) {
        // without room for the plan's scratch the shard keeps the host planner
        // (ready() stays false); what was allocated is freed with the shard
        const size_t cb = (size_t)dp.capBatches;
        unsigned char* temp = nullptr;
        if ((rc = dev_alloc(sh, &dp.keyIn, (size_t)dp.capRows)) || (rc = dev_alloc(sh, &dp.keyOut, (size_t)dp.capRows)) ||
            (rc = dev_alloc(sh, &dp.sorted, (size_t)dp.capRows)) ||
            (rc = dev_alloc(sh, &dp.rowsTmp, (size_t)dp.capRows + 64)) ||
            (rc = dev_alloc(sh, &dp.offTmp, (size_t)dp.capRows + 64)) || (rc = dev_alloc(sh, &dp.cost, cb)) ||
            (rc = dev_alloc(sh, &dp.costSorted, cb)) || (rc = dev_alloc(sh, &dp.idx, cb)) ||
            (rc = dev_alloc(sh, &dp.perm, cb)) || (rc = dev_alloc(sh, &temp, dp.tempBytes)))
            (void)hipGetLastError();
        dp.temp = rc ? nullptr : temp;   // (marks the scratch ready: written last)
    }
    sh->bsc.next = sh->bsc.queue + slots * NS;
    sh->bsc.nStride = (int64_t)NS;
    sh->bsc.arcHit = nullptr;
    sh->bsc.mStride = (int64_t)mStride;
    // (no room for the flags: no filter, the post kernel reads every in-arc)
    sh->bsc.hitLds = 0;
    if (filter && dev_alloc(sh, &sh->bsc.arcHit, roundB * (mStride / 32))) (void)hipGetLastError();
    sh->bsc.predCnt = nullptr;
    if (pe->tu.debug && (rc = dev_alloc(sh, &sh->bsc.predCnt, 2))) return rc;
    sh->bsc.LB = nullptr;
    sh->bsc.redo = nullptr;
    sh->bsc.redoRun = 0;
    sh->bsc.bits = nullptr;
    if (bitBytes && (rc = dev_alloc(sh, &sh->bsc.bits, slots * bitBytes / 4))) return rc;
    sh->bsc.laneOff = sh->dLaneOff;
    if ((rc = ensure_tie(pe, sh))) return rc;
    sh->batchReady = true;
    // SHDPE_POST_SPLIT=1: the two parts without a tune, where their label arrays fit
    if (plan.postSplit && !ensure_label_arrays(pe, sh)) {
        plan.postSplit = false;
        plan.post = plan.redo;
    }
    return SHD_PE_OK;
}

static int ensure_dense(ShdPe* pe, Shard* sh) {
    if (sh->dW) return SHD_PE_OK;
    const int64_t n = pe->hg.n;
    const int64_t R = std::max<int32_t>(1, sh->rowCount);
    int rc;
    double* w;                      // (dW marks the whole set ready: written last)
    // rows per batch: D (f64) + P (i32) per row
    const int64_t budget = (int64_t)(pe->tu.denseBatchGB * (double)(1LL << 30));
    int64_t rows = std::max<int64_t>(64, budget / (n * 12));
    rows = std::min<int64_t>(rows, R);
    if ((rc = dev_alloc(sh, &w, (size_t)(n * n))) || (rc = dev_alloc(sh, &sh->dRl, (size_t)(n * n))) ||
        (rc = dev_alloc(sh, &sh->dD, (size_t)(rows * n))) || (rc = dev_alloc(sh, &sh->dP, (size_t)(rows * n))) ||
        (rc = dev_alloc(sh, &sh->dRowA, (size_t)rows)) || (rc = dev_alloc(sh, &sh->dRowB, (size_t)rows)) ||
        (rc = dev_alloc(sh, &sh->dRowAmbD, (size_t)rows)) || (rc = dev_alloc(sh, &sh->dAny, 4)) ||
        (rc = dev_alloc(sh, &sh->dChunkEpoch, (size_t)((rows / 16 + 1) * (n / 16 + 1)))))
        return rc;
    sh->dW = w;
    sh->denseRows = (int32_t)rows;
    launch_dense_build(sh->dg, sh->dW, sh->dRl, n, pe->hg.nArcs(), sh->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(sh->stream));
    return SHD_PE_OK;
}

float shdpe::elapsed(hipEvent_t a, hipEvent_t b) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, a, b);
    return ms;
}

// Kernel counters of k_batch_rows (SHD_PE_DEBUG_COUNTERS): phase cycles,
// re-visits, jump rounds, per-batch cost spread.
static void print_batch_debug(ShdPe* pe, Shard* sh, const BatchLaunch& relax, const int32_t* d0, int32_t nB) {
    double ph = 0, pr = 0, kc[5] = {0, 0, 0, 0, 0}, arcsP = 0, lanesP = 0, bmax = 0, bmean = 0, cand = 0,
           walks = 0;
    long ambB = 0, rep = 0;
    double tMin = 1e30, tMax = 0, tSum = 0, tSq = 0;
    for (int32_t i = 0; i < nB; ++i) {
        const int32_t* d = d0 + 16 * i;
        ph += d[0];
        ambB += d[3] != 0;
        rep += d[15];
        pr += d[4];
        double tb = 0;
        for (int k = 0; k < 3; ++k) { kc[k] += 1024.0 * d[5 + k]; tb += 1024.0 * d[5 + k]; }
        kc[3] += 1024.0 * d[11]; tb += 1024.0 * d[11];
        kc[4] += 1024.0 * d[8]; tb += 1024.0 * d[8];
        tMin = std::min(tMin, tb); tMax = std::max(tMax, tb); tSum += tb; tSq += tb * tb;
        arcsP += 16.0 * d[9];
        bmax += 1024.0 * d[12]; bmean += 1024.0 * d[13]; cand += d[14];
        lanesP += d[10];
        walks += 1024.0 * d[2];
    }
    const double mean = tSum / std::max(nB, 1);
    const double sd = std::sqrt(std::max(0.0, tSq / std::max(nB, 1) - mean * mean));
    std::fprintf(stderr, "[shdpe] shard %d batch relax Mcycles/batch: sum over phases of group-busy max=%.2f mean=%.2f | candidates/batch=%.0f\n",
                 sh->gindex, bmax / nB / 1e6, bmean / nB / 1e6, cand / nB);
    std::fprintf(stderr, "[shdpe] batch arc-visits/batch=%.0f (%.2f x nArcs) active lanes/proc=%.2f\n",
                 arcsP / nB, arcsP / nB / (double)pe->hg.nArcs(), lanesP / std::max(pr, 1.0));
    std::fprintf(stderr, "[shdpe] batch Mcycles/batch: relax=%.2f pred=%.2f labels+write=%.2f (walks %.2f) tie-export=%.2f tail=%.2f | "
                 "per-batch total min=%.2f mean=%.2f max=%.2f sd=%.2f\n", kc[0] / nB / 1e6, kc[1] / nB / 1e6,
                 kc[2] / nB / 1e6, walks / nB / 1e6, kc[3] / nB / 1e6, kc[4] / nB / 1e6, tMin / 1e6, mean / 1e6,
                 tMax / 1e6, sd / 1e6);
    // SHDPE_DIAG_WHY builds: per reason bit, the batches it fired in
    long why[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool anyWhy = false;
    for (int32_t i = 0; i < nB; ++i)
        for (int k = 0; k < 8; ++k)
            if ((d0[16 * i + 1] >> k) & 1) { ++why[k]; anyWhy = true; }
    if (anyWhy)
        std::fprintf(stderr, "[shdpe] batch why: failed=%ld viol-ondemand=%ld viol-full=%ld noparent=%ld "
                     "ambiguous=%ld deep=%ld fullpass=%ld relax-flag=%ld\n", why[0], why[1], why[2],
                     why[3], why[4], why[5], why[6], why[7]);
    std::fprintf(stderr, "[shdpe] batch LB=%d batches=%d grid=%d delta=%.3f | phases/batch=%.1f "
                 "vertex-procs/batch=%.0f (%.2f per vertex) | tie batches=%ld repairs=%ld\n",
                 relax.lb, nB, relax.grid, relax.delta, ph / nB, pr / nB,
                 pr / nB / pe->hg.n, ambB, rep);
}

// SHDPE_DUMP_BATCHES=<file>: per batch its rows (table positions, -1 pads),
// hub offsets, kernel counters, hub-group distances and, last, the offsets the
// kernel ran with per (batch, lane), for offline batch-cost models
// (tools/batch_cost.py)
static void dump_batches(const ShdPe* pe, const std::vector<int32_t>& order, const std::vector<double>& laneOff,
                         const std::vector<int32_t>& dbg, int32_t nB, int32_t LB) {
    const char* f = std::getenv("SHDPE_DUMP_BATCHES");
    FILE* fp = f ? std::fopen(f, "wb") : nullptr;
    if (!fp) return;
    const int32_t hdr[2] = {nB, LB};
    std::fwrite(hdr, 4, 2, fp);
    std::fwrite(order.data(), 4, order.size(), fp);
    std::fwrite(dbg.data(), 4, dbg.size(), fp);
    const int64_t nOff = (int64_t)pe->rowOff.size();
    std::fwrite(&nOff, 8, 1, fp);
    std::fwrite(pe->rowOff.data(), 8, pe->rowOff.size(), fp);
    // batch order 2: the hub-group distances and the latency unit of batch_order_cost
    const int32_t nGroups = pe->hubGroups.G;
    std::fwrite(&nGroups, 4, 1, fp);
    std::fwrite(&pe->hg.meanArcLatency, 8, 1, fp);
    std::fwrite(pe->hubGroups.dist.data(), 8, pe->hubGroups.dist.size(), fp);
    std::fwrite(laneOff.data(), 8, laneOff.size(), fp);     // [nB * LB], after what older readers read
    std::fclose(fp);
}

static void print_sparse_debug(ShdPe* pe, Shard* sh, const int32_t* dbg, int32_t cnt) {
    double ph = 0, cy[4] = {0, 0, 0, 0}, sub[4] = {0, 0, 0, 0};
    int phMax = 0, jMax = 0, mis = 0, am = 0;
    long jSum = 0;
    for (int32_t i = 0; i < cnt; ++i) {
        const int32_t* d = dbg + 16 * i;
        ph += d[0]; phMax = std::max(phMax, d[0]);
        jMax = std::max(jMax, d[1]); jSum += d[1];
        mis += d[2] != 0; am += d[3] != 0;
        for (int k = 0; k < 4; ++k) cy[k] += 16.0 * d[4 + k];
        for (int k = 0; k < 4; ++k) sub[k] += 16.0 * d[8 + k];
    }
    std::fprintf(stderr,
                 "[shdpe] shard %d sparse rows=%d phases mean=%.1f max=%d | mismatch rows=%d "
                 "jacobi rounds sum=%ld max=%d | ambiguous rows=%d | delta=%.3f | "
                 "kcycles/row scan=%.1f relax=%.1f final=%.1f write=%.1f | "
                 "cyc/phase bits=%.0f resv=%.0f light=%.0f heavy=%.0f\n",
                 sh->gindex, cnt, ph / cnt, phMax, mis, jSum, jMax, am, sh->cfg.delta,
                 cy[0] / cnt / 1e3, cy[1] / cnt / 1e3, cy[2] / cnt / 1e3, cy[3] / cnt / 1e3,
                 sub[0] / ph, sub[1] / ph, sub[2] / ph, sub[3] / ph);
    (void)pe;
}

// k_exact_rows counters: per row pops, pushes and cycles per pop segment.
static void print_exact_debug(Shard* sh, const std::vector<int32_t>& rows, int32_t nTie) {
    std::vector<long long> x(rows.size() * 8);
    if (hipMemcpy(x.data(), sh->dXdbg, x.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return;
    for (size_t i = 0; i < rows.size(); ++i) {
        const long long* c = &x[i * 8];
        const double p = (double)std::max<long long>(c[5], 1);
        std::fprintf(stderr, "[shdpe] exact row %d (%s): pops=%lld pushes+mods=%lld heap_end=%lld | "
                     "cyc/pop top=%.0f sink=%.0f arcs=%.0f push=%.0f fence=%.0f total=%.0f\n",
                     rows[i], (int32_t)i < nTie ? "early" : "full", c[5], c[6], c[7], c[0] / p,
                     c[1] / p, c[2] / p, c[3] / p, c[4] / p, (c[0] + c[1] + c[2] + c[3] + c[4]) / p);
    }
}

// SHDPE_TIE_CORRUPT (tests): after the relevance scan, halve the exported
// distances of the first early-stop slot that still needs the emulation --
// what a slot filled from another source's distance array would hold.  The
// exact kernel's consistency check must catch it (rowsTieRepaired).
static void corrupt_tie_slot(ShdPe* pe, Shard* sh, const std::vector<int32_t>& slots, int32_t nTie) {
    std::vector<double> thr((size_t)sh->tie.cap), d((size_t)pe->hg.n);
    if (hipStreamSynchronize(sh->stream) != hipSuccess ||
        hipMemcpy(thr.data(), sh->tie.thr, thr.size() * 8, hipMemcpyDeviceToHost) != hipSuccess)
        return;
    for (int32_t i = 0; i < nTie; ++i) {
        const int sl = slots[i];
        if (!(thr[(size_t)sl] > 0.0)) continue;
        double* dd = sh->tie.D + (size_t)sl * (size_t)sh->tie.n;
        if (hipMemcpy(d.data(), dd, d.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return;
        // 1: another source's array (halved distances); 2: an array whose
        // own source is not at 0 (every distance shifted)
        for (double& x : d) x = pe->tu.tieCorrupt == 2 ? x + 1.0 : x * 0.5;
        (void)hipMemcpy(dd, d.data(), d.size() * 8, hipMemcpyHostToDevice);
        return;
    }
}

// The batch scratch for a launch over the batches at `rows` (inside
// dBatchRows): the lane offsets are those of the same entries of dLaneOff.
static BatchScratch scratch_at(const Shard* sh, const int32_t* rows) {
    BatchScratch bs = sh->bsc;
    bs.laneOff = sh->dLaneOff + (rows - sh->dBatchRows);
    return bs;
}

// One chunk's rows for the exact stage, as the chunk's relax stage leaves them.
struct ExactWork {
    std::vector<int32_t> rows;       // table positions: early-stop tie rows first, then full-emulation rows
    std::vector<int32_t> slots;      // per row its tie slot, -1 full emulation (empty: no early-stop row)
    std::vector<int32_t> denseIdx;   // dense tie rows: their row of D / P (one dense chunk only)
    void clear() { rows.clear(); slots.clear(); denseIdx.clear(); }
};

// Rows a sparse relax kernel flagged (amb[i] != 0; ids[i] < 0 pads a batch):
// early-stop tie rows (amb = 2 + slot) first (k_tie_write takes that
// prefix), then rows needing the full emulation (amb = 1)
static void classify_rows(const int32_t* ids, size_t count, const uint8_t* amb, ExactWork& x) {
    std::vector<int32_t> fullRows;
    for (size_t i = 0; i < count; ++i) {
        if (ids[i] < 0 || !amb[i]) continue;
        if (amb[i] >= 2) {
            x.rows.push_back(ids[i]);
            x.slots.push_back(amb[i] - 2);
        } else {
            fullRows.push_back(ids[i]);
        }
    }
    if (!x.slots.empty()) {
        x.rows.insert(x.rows.end(), fullRows.begin(), fullRows.end());
        x.slots.resize(x.rows.size(), -1);
    } else {
        x.rows.swap(fullRows);
    }
}

// ---- relax stages: the rows at `pos` (cnt of them, already in dRows) ----------

static int relax_direct(ShdPe*, Shard* sh, const int32_t*, int32_t cnt, ExactWork&) {
    ShdPeStats& st = sh->stats;
    HIPCHK(hipEventRecord(sh->evA, sh->stream));
    launch_direct_rows(sh->dg, sh->tab, sh->dRows, cnt, sh->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(sh->evB, sh->stream));
    HIPCHK(hipEventSynchronize(sh->evB));
    st.msDirectKernel += elapsed(sh->evA, sh->evB);
    st.launchesDirect++;
    return SHD_PE_OK;
}

static int relax_dense(ShdPe* pe, Shard* sh, const int32_t* pos, int32_t cnt, ExactWork& x) {
    ShdPeStats& st = sh->stats;
    int rc;
    if ((rc = ensure_dense(pe, sh))) return rc;
    std::vector<uint8_t> amb;
    for (int32_t d0 = 0; d0 < cnt; d0 += sh->denseRows) {
        const int32_t dc = std::min(sh->denseRows, cnt - d0);
        HIPCHK(hipEventRecord(sh->evA, sh->stream));
        int sweeps = 0;
        double flops = 0.0;
        if (launch_dense_rows(sh->dg, sh->tab, sh->dW, sh->dRl, sh->dD, sh->dP, sh->dRowA, sh->dRowB,
                              sh->dRowAmbD, sh->dAny, sh->dChunkEpoch, sh->dRows + d0, dc, pe->hg.n,
                              pe->tu, sh->stream, &sweeps, &flops, DENSE_ALL))
            return SHD_PE_EHIP;
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(sh->evB, sh->stream));
        amb.resize(dc);
        HIPCHK(hipMemcpyAsync(amb.data(), sh->dRowAmbD, dc, hipMemcpyDeviceToHost, sh->stream));
        HIPCHK(hipStreamSynchronize(sh->stream));
        st.msDenseKernel += elapsed(sh->evA, sh->evB);
        st.launchesDense++;
        st.denseSweeps += sweeps;
        st.denseFlops += flops;
        for (int32_t i = 0; i < dc; ++i)
            if (amb[i]) {
                x.rows.push_back(pos[d0 + i]);
                if (dc == cnt) x.denseIdx.push_back(i);   // D / P still hold the row
            }
    }
    return SHD_PE_OK;
}

// Split kernels: rounds of batches: relax all of them, then the post kernel
// over the same batches (their dist arrays persist in HBM)
// (the post kernel may run another variant than the relax).  A timed trial
// gets the parts' times.
// roundHook (shd_pe_get_paths; null otherwise): called after each round's
// post kernel and tie export, while the round's dist arrays and ambiguity
// bytes are still in place, with the round's first batch and batch count.
using RoundHook = std::function<int(int32_t r0, int32_t rn)>;

// The post launches of a round: the one post kernel, or its two parts and the
// redo launch (BatchPlan).
struct PostLaunches {
    BatchLaunch post{}, label{}, redo{};
    bool split = false;
};

static int batch_rounds(ShdPe* pe, Shard* sh, const BatchLaunch& relax, const PostLaunches& pl, int32_t nB,
                        BatchTrial* trial, const RoundHook* roundHook = nullptr) {
    const int LB = relax.lb;
    const bool timed = trial && trial->timed;
    const bool noTable = trial && trial->noTable;
    // (shd_pe_get_paths' pass stores no row: PART 4, the one post kernel)
    const bool split = pl.split && !noTable && sh->postSplitOk && sh->bsc.LB && sh->bsc.redo;
    int rc;
    for (int32_t r0 = 0; r0 < nB; r0 += sh->batchRound) {
        const int32_t rn = std::min(sh->batchRound, nB - r0);
        const size_t ro = (size_t)r0 * LB;
        sh->roundsRun++;
        sh->batchesRun += rn;
        int32_t* const dbgR = sh->dDbg ? sh->dDbg + 16 * r0 : nullptr;
        const BatchScratch bs = scratch_at(sh, sh->dBatchRows + ro);
        auto launch = [&](const BatchLaunch& cfg, int part, const BatchScratch& b) {
            if (hipMemsetAsync(sh->bsc.next, 0, 4, sh->stream) != hipSuccess) return SHD_PE_EHIP;
            launch_batch_rows(sh->dg, sh->tab, b, sh->dBatchRows + ro, rn, sh->dBatchAmb + ro, cfg, dbgR, sh->dTie,
                              sh->stream, part);
            return SHD_PE_OK;
        };
        if (timed) HIPCHK(hipEventRecord(sh->evP[0], sh->stream));
        if ((rc = launch(relax, 1, bs))) return rc;
        // tests only (SHDPE_TUNE_FAIL_WPE): the relax variant of that wave
        // count flags every batch failed, as a miscompiled variant would
        if (pe->tu.failWpe && relax.wpe == pe->tu.failWpe)
            HIPCHK(hipMemsetAsync(sh->bsc.flags, 1, (size_t)rn * 4, sh->stream));
        if (timed) HIPCHK(hipEventRecord(sh->evP[1], sh->stream));
        // the post kernel's deferred tie export of this round (the round's dist
        // arrays persist until the next round's relax)
        if (sh->tie.req)
            HIPCHK(hipMemsetD32Async((hipDeviceptr_t)sh->tie.round, r0 / sh->batchRound, 1, sh->stream));
        if (!split) {
            if ((rc = launch(pl.split ? pl.redo : pl.post, noTable ? 4 : 2, bs))) return rc;
            if (timed) HIPCHK(hipEventRecord(sh->evP[2], sh->stream));
        } else {
            // predecessor part, label part, then the one post kernel over the
            // batches the label part listed (a grid that exits at once when
            // there are none): ordered by the stream alone
            if ((rc = launch(pl.post, 5, bs))) return rc;
            if (timed) HIPCHK(hipEventRecord(sh->evP[2], sh->stream));
            HIPCHK(hipMemsetAsync(sh->bsc.redo, 0, 4, sh->stream));
            if ((rc = launch(pl.label, 6, bs))) return rc;
            BatchScratch br = bs;
            br.redoRun = 1;
            if ((rc = launch(pl.redo, 2, br))) return rc;
        }
        if (timed) HIPCHK(hipEventRecord(sh->evP[3], sh->stream));
        if (sh->tie.req)
            launch_tie_export(sh->dg, sh->bsc, LB, sh->tie, r0 / sh->batchRound, sh->dBatchAmb + ro,
                              sh->numCUs * 4, pe->tu.tieCorrupt == 3 ? 0 : -1, sh->stream);
        if (roundHook && (rc = (*roundHook)(r0, rn))) return rc;
        if (timed) {
            HIPCHK(hipEventSynchronize(sh->evP[3]));
            trial->msRelax += elapsed(sh->evP[0], sh->evP[1]);
            trial->msPost += elapsed(sh->evP[1], sh->evP[2]);
            trial->msLabel += elapsed(sh->evP[2], sh->evP[3]);
        }
    }
    return SHD_PE_OK;
}

// The launches to use now: the plan's picks, or those of the tune's trial.
static const BatchLaunch& relax_launch(const Shard* sh, const BatchTrial* trial) {
    return trial ? trial->relax : sh->plan.relax;
}
static PostLaunches post_launches(const Shard* sh, const BatchTrial* trial) {
    if (trial) return PostLaunches{trial->post, trial->label, trial->postSplit ? trial->redo : trial->post,
                                   trial->postSplit};
    const BatchPlan& p = sh->plan;
    return PostLaunches{p.post, p.label, p.redo, p.postSplit};
}

// (batchOrder / roundHook: shd_pe_get_paths -- batch_order of these rows, which
// that caller needs first, and batch_rounds' per-round hook; split kernels only)
static int relax_batched(ShdPe* pe, Shard* sh, const int32_t* pos, int32_t cnt, ExactWork& x,
                         BatchTrial* trial, const std::vector<int32_t>* batchOrder = nullptr,
                         const RoundHook* roundHook = nullptr) {
    ShdPeStats& st = sh->stats;
    int rc;
    if ((rc = ensure_batch(pe, sh))) return rc;
    const BatchLaunch& relax = relax_launch(sh, trial);
    int32_t nB = 0;
    const int offKind = pe->tu.laneOffset != 0;
    const bool byCost = !batchOrder && !pe->hubGroups.empty();
    // batch order 2 composes its plan on the device, from the positions in
    // dRows (the plan kernels, pe_plan_dev.hip): the host neither plans nor
    // uploads before the relax launch, and reads `order` back behind the
    // kernels.  (SHDPE_DEVICE_PLAN=0, tests: batch_order_cost, the reference.)
    const bool onDevice = byCost && sh->dplan.ready() && pe->tu.devicePlan != 0;
    std::vector<double> laneOff;     // per entry of `order`: they depend on who shares the batch
    std::vector<int32_t> order;
    if (onDevice) {
        nB = (cnt + relax.lb - 1) / relax.lb;
        order.resize((size_t)nB * (size_t)relax.lb);
        // the control words of the call go with the plan's last kernel.  The tie
        // slots' deferred-export requests: round -1, as below
        PlanControl ctl;
        ctl.next = sh->bsc.next;
        ctl.redo = sh->bsc.redo;
        ctl.predCnt = sh->bsc.predCnt;
        ctl.tieCount = sh->tie.cap > 0 ? sh->tie.count : nullptr;
        ctl.tieReq = sh->tie.req;
        ctl.tieReqWords = sh->tie.req ? (int64_t)sh->tie.cap * 4 : 0;
        ctl.dbg = sh->dDbg;
        ctl.dbgWords = sh->dDbg ? (int64_t)nB * 16 : 0;
        if ((rc = launch_plan_dev(sh->dplan, sh->dRows, cnt, relax.lb, offKind, sh->dBatchRows, sh->dLaneOff, ctl,
                                  sh->stream)))
            return rc;
    } else {
        order = batchOrder ? *batchOrder
                : byCost   ? batch_order_cost(pe->rank, pe->rowOff, pe->hubGroups, pe->hg.meanArcLatency, relax.lb,
                                              pos, cnt, nB, nullptr, &laneOff, offKind)
                           : batch_order(pe->rank, pe->rowOff, relax.lb, pos, cnt, nB);
        if (!byCost) laneOff = lane_offsets(pe->hubGroups, pe->rowOff, order, relax.lb, offKind);
        nB = (int32_t)(order.size() / (size_t)relax.lb);
        HIPCHK(hipMemcpyAsync(sh->dBatchRows, order.data(), order.size() * 4, hipMemcpyHostToDevice, sh->stream));
        HIPCHK(hipMemcpyAsync(sh->dLaneOff, laneOff.data(), laneOff.size() * 8, hipMemcpyHostToDevice, sh->stream));
        if (sh->dDbg) HIPCHK(hipMemsetAsync(sh->dDbg, 0, (size_t)nB * 64, sh->stream));
        if (sh->bsc.predCnt) HIPCHK(hipMemsetAsync(sh->bsc.predCnt, 0, 16, sh->stream));
        if (sh->bsc.redo) HIPCHK(hipMemsetAsync(sh->bsc.redo, 0, 8, sh->stream));
        if (sh->tie.cap > 0) HIPCHK(hipMemsetAsync(sh->tie.count, 0, 4, sh->stream));
        // the slots' deferred-export requests: round -1, which no round's k_tie_export
        // serves.  A slot the post kernel fills in line (its second attempt: a deep
        // tree with ties) gets no request, and the words an earlier call -- or the
        // allocator -- left there would name a batch of this call's round
        if (sh->tie.req) HIPCHK(hipMemsetAsync(sh->tie.req, 0xFF, (size_t)sh->tie.cap * 16, sh->stream));
        HIPCHK(hipMemsetAsync(sh->bsc.next, 0, 4, sh->stream));
    }
    HIPCHK(hipEventRecord(sh->evA, sh->stream));
    if (!relax.split)
        launch_batch_rows(sh->dg, sh->tab, scratch_at(sh, sh->dBatchRows), sh->dBatchRows, nB, sh->dBatchAmb, relax,
                          sh->dDbg, sh->dTie, sh->stream, 0);
    else if ((rc = batch_rounds(pe, sh, relax, post_launches(sh, trial), nB, trial, roundHook)))
        return rc;
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(sh->evB, sh->stream));
    std::vector<uint8_t> amb(order.size());
    HIPCHK(hipMemcpyAsync(amb.data(), sh->dBatchAmb, order.size(), hipMemcpyDeviceToHost, sh->stream));
    if (onDevice)                    // (the kernels only read dBatchRows: still the plan's rows)
        HIPCHK(hipMemcpyAsync(order.data(), sh->dBatchRows, order.size() * 4, hipMemcpyDeviceToHost, sh->stream));
    int32_t redone[2] = {0, 0};      // [1]: batches of this call that took the redo launch
    if (sh->bsc.redo) HIPCHK(hipMemcpyAsync(redone, sh->bsc.redo, 8, hipMemcpyDeviceToHost, sh->stream));
    HIPCHK(hipStreamSynchronize(sh->stream));
    sh->redoBatches += redone[1];
    st.msSparseKernel += elapsed(sh->evA, sh->evB);
    st.launchesSparse++;
    classify_rows(order.data(), order.size(), amb.data(), x);
    if (sh->dDbg) {
        std::vector<int32_t> dbg((size_t)nB * 16);
        HIPCHK(hipMemcpy(dbg.data(), sh->dDbg, dbg.size() * 4, hipMemcpyDeviceToHost));
        print_batch_debug(pe, sh, relax, dbg.data(), nB);
        std::fprintf(stderr, "[shdpe] shard %d batch plan by the %s\n", sh->gindex,
                     onDevice ? "plan kernels" : batchOrder ? "caller" : "host planner");
        if (onDevice) {              // the dump carries the plan the kernels ran with
            laneOff.resize(order.size());
            HIPCHK(hipMemcpy(laneOff.data(), sh->dLaneOff, laneOff.size() * 8, hipMemcpyDeviceToHost));
        }
        dump_batches(pe, order, laneOff, dbg, nB, relax.lb);
        if (sh->bsc.predCnt) {
            unsigned long long pc[2] = {0, 0};
            HIPCHK(hipMemcpy(pc, sh->bsc.predCnt, 16, hipMemcpyDeviceToHost));
            sh->predClaimed += (int64_t)pc[0];
            sh->predGathered += (int64_t)pc[1];
            std::fprintf(stderr, "[shdpe] on-demand predecessor pass in-arcs/batch: claimed=%.0f gathered=%.0f "
                         "(%.3f / %.3f x nArcs; filter %s)\n", (double)pc[0] / std::max(nB, 1),
                         (double)pc[1] / std::max(nB, 1), (double)pc[0] / std::max(nB, 1) / (double)pe->hg.nArcs(),
                         (double)pc[1] / std::max(nB, 1) / (double)pe->hg.nArcs(), sh->bsc.arcHit ? "on" : "off");
        }
    }
    return SHD_PE_OK;
}

static int relax_sparse(ShdPe* pe, Shard* sh, const int32_t* pos, int32_t cnt, ExactWork& x) {
    ShdPeStats& st = sh->stats;
    int rc;
    if ((rc = ensure_tie(pe, sh))) return rc;
    if (sh->dTie) HIPCHK(hipMemsetAsync(sh->tie.count, 0, 4, sh->stream));
    HIPCHK(hipEventRecord(sh->evA, sh->stream));
    launch_sparse_rows(sh->dg, sh->tab, sh->sc, sh->dRows, cnt, sh->dRowAmbig, sh->cfg,
                       sh->dDbg, sh->dTie, sh->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(sh->evB, sh->stream));
    std::vector<uint8_t> amb(cnt);
    HIPCHK(hipMemcpyAsync(amb.data(), sh->dRowAmbig, cnt, hipMemcpyDeviceToHost, sh->stream));
    HIPCHK(hipStreamSynchronize(sh->stream));
    st.msSparseKernel += elapsed(sh->evA, sh->evB);
    st.launchesSparse++;
    classify_rows(pos, (size_t)cnt, amb.data(), x);
    if (sh->dDbg) {
        std::vector<int32_t> dbg((size_t)cnt * 16);
        HIPCHK(hipMemcpy(dbg.data(), sh->dDbg, dbg.size() * 4, hipMemcpyDeviceToHost));
        print_sparse_debug(pe, sh, dbg.data(), cnt);
    }
    return SHD_PE_OK;
}

// One chunk's relax stage, by the shard's mode.  (trial: shd_pe_tune's
// launches for the batched kernel, null otherwise.)
static int relax_stage(ShdPe* pe, Shard* sh, const int32_t* pos, int32_t cnt, ExactWork& x,
                       BatchTrial* trial) {
    if (pe->mode == 2) return relax_direct(pe, sh, pos, cnt, x);
    if (pe->opt.forceMode == 3 || pe->hg.latFold) {
        // (latFold multigraphs: the reported latency is a fold of other
        // edges' latencies than the distance's -- the exact emulation
        // carries it as a label, so every row takes that path)
        x.rows.assign(pos, pos + cnt);
        return SHD_PE_OK;
    }
    if (pe->mode == 3) return relax_dense(pe, sh, pos, cnt, x);
    if (pe->batched) return relax_batched(pe, sh, pos, cnt, x, trial);
    return relax_sparse(pe, sh, pos, cnt, x);
}

// ---- exact stage: the igraph emulation of the rows a relax stage left ---------

// The shard's exact emulation is k_exact_dense (~n arcs per pop: the
// workgroup-wide scan) rather than k_exact_rows.  (Rows with tie slots in
// dSlots take k_exact_rows all the same: exact_general.)
static bool dense_emulation(const ShdPe* pe) {
    return pe->mode == 3 && pe->opt.forceMode != 3 && !pe->hg.latFold;
}

// k_exact_dense's per-slot lists, allocated at its first use.
static int ensure_xlist(Shard* sh) {
    if (sh->dXList) return SHD_PE_OK;
    return dev_alloc(sh, &sh->dXList, (size_t)sh->exactGrid * (size_t)sh->sc.stride *
                                          (size_t)exact_dense_list_bytes());
}

// The emulation of the first n rows in dRows: in full, but for those of them
// with a slot in dSl (k_exact_rows only; null: none), which stop early.
static void launch_emulation(ShdPe* pe, Shard* sh, int32_t n, bool dense, const int32_t* dSl,
                             long long* dbg) {
    if (dense)
        launch_exact_dense(sh->dg, sh->tab, sh->sc, sh->dRows, n, sh->exactGrid, sh->exactHc,
                           sh->dXList, nullptr, sh->tie, nullptr, sh->stream);
    else
        launch_exact_rows(sh->dg, sh->tab, sh->sc, sh->dRows, n, sh->exactGrid, sh->exactHc,
                          pe->tu.exactHc > 0, dSl, sh->tie, dbg, sh->stream);
}

// The relevance scan of the first nTie rows in dRows (their slots in dSlots;
// `slots`: the host's copy), and the test hook right after it.
static void scan_tie_slots(ShdPe* pe, Shard* sh, const std::vector<int32_t>& slots, int32_t nTie) {
    launch_tie_scan(sh->dg, sh->dRows, sh->dSlots, nTie, sh->tie, sh->stream);
    if (pe->tu.tieCorrupt == 1 || pe->tu.tieCorrupt == 2) corrupt_tie_slot(pe, sh, slots, nTie);
}

// Early-stop rows whose slot failed the exact kernel's consistency check
// (thr = NaN: the exported distances are not this row's): k_tie_write
// skipped them.  Reads thr[0, nThr) back and appends those of rows[0, nTie)
// to `redo`; repair_tie_rows recomputes them by the full emulation.
static int failed_tie_rows(Shard* sh, const int32_t* rows, const int32_t* slots, int32_t nTie,
                           int32_t nThr, std::vector<int32_t>& redo) {
    std::vector<double> thr((size_t)nThr);
    HIPCHK(hipMemcpyAsync(thr.data(), sh->tie.thr, thr.size() * 8, hipMemcpyDeviceToHost, sh->stream));
    HIPCHK(hipStreamSynchronize(sh->stream));
    for (int32_t i = 0; i < nTie; ++i)
        if (std::isnan(thr[(size_t)slots[i]])) redo.push_back(rows[i]);
    return SHD_PE_OK;
}

static int repair_tie_rows(ShdPe* pe, Shard* sh, const std::vector<int32_t>& redo, bool dense) {
    if (redo.empty()) return SHD_PE_OK;
    std::fprintf(stderr, "[shdpe] shard %d: %zu %searly-stop tie row(s) failed the slot "
                 "consistency check; recomputed by the full emulation\n",
                 sh->gindex, redo.size(), dense ? "dense " : "");
    HIPCHK(hipMemcpyAsync(sh->dRows, redo.data(), redo.size() * 4, hipMemcpyHostToDevice, sh->stream));
    launch_emulation(pe, sh, (int32_t)redo.size(), dense, nullptr, nullptr);
    HIPCHK(hipGetLastError());
    sh->stats.rowsTieRepaired += (int64_t)redo.size();
    return SHD_PE_OK;
}

// Dense tie rows with early stop (round 6; undirected graphs whose rows
// fit one dense chunk, so D / P still hold them): in groups of the
// tie slots, each row's slot filled from D / P (k_dense_tie_export),
// the relevance scan, the emulation only until the row's tied
// predecessors are popped (k_exact_dense) and k_tie_write.  A slot
// failing the emulation's consistency check is redone in full.
static int exact_dense_early(ShdPe* pe, Shard* sh, const ExactWork& x) {
    ShdPeStats& st = sh->stats;
    int rc;
    if (!sh->dDenseIdx && (rc = dev_alloc(sh, &sh->dDenseIdx, (size_t)sh->rowsCap))) return rc;
    if ((rc = ensure_xlist(sh))) return rc;
    const int32_t cap = sh->tie.cap;
    std::vector<int32_t> slots(cap), redo;
    for (int32_t k = 0; k < cap; ++k) slots[k] = k;
    HIPCHK(hipMemcpyAsync(sh->dSlots, slots.data(), (size_t)cap * 4, hipMemcpyHostToDevice, sh->stream));
    HIPCHK(hipEventRecord(sh->evA, sh->stream));
    for (size_t g0 = 0; g0 < x.rows.size(); g0 += (size_t)cap) {
        const int32_t k = (int32_t)std::min<size_t>(cap, x.rows.size() - g0);
        HIPCHK(hipMemcpyAsync(sh->dRows, x.rows.data() + g0, (size_t)k * 4, hipMemcpyHostToDevice, sh->stream));
        HIPCHK(hipMemcpyAsync(sh->dDenseIdx, x.denseIdx.data() + g0, (size_t)k * 4, hipMemcpyHostToDevice,
                              sh->stream));
        HIPCHK(hipMemsetAsync(sh->tie.thr, 0, (size_t)k * 8, sh->stream));
        launch_dense_tie_export(sh->dg, sh->dD, sh->dP, pe->hg.n, sh->dDenseIdx, sh->dRows, sh->tie,
                                k, sh->stream);
        scan_tie_slots(pe, sh, slots, k);
        // rows of unequal early-stop cost: taken from a counter
        HIPCHK(hipMemsetAsync(sh->tie.count + 2, 0, 4, sh->stream));
        launch_exact_dense(sh->dg, sh->tab, sh->sc, sh->dRows, k, sh->exactGrid, sh->exactHc,
                           sh->dXList, sh->dSlots, sh->tie, sh->tie.count + 2, sh->stream);
        launch_tie_write(sh->dg, sh->tab, sh->dRows, sh->dSlots, k, sh->tie, sh->stream);
        HIPCHK(hipGetLastError());
        if ((rc = failed_tie_rows(sh, x.rows.data() + g0, slots.data(), k, k, redo))) return rc;
        st.rowsTieEarly += k;
    }
    if ((rc = repair_tie_rows(pe, sh, redo, true))) return rc;
    HIPCHK(hipEventRecord(sh->evB, sh->stream));
    HIPCHK(hipEventSynchronize(sh->evB));
    st.msExactKernel += elapsed(sh->evA, sh->evB);
    st.launchesExact++;
    st.rowsExact += (int64_t)x.rows.size();
    return SHD_PE_OK;
}

// The general form: one emulation launch over the early-stop rows (slots
// from the sparse kernels' tie export) and the full rows together, then
// k_tie_write over the early-stop prefix; the cross-check's repairs after
// the timed window.
static int exact_general(ShdPe* pe, Shard* sh, const ExactWork& x) {
    ShdPeStats& st = sh->stats;
    int rc;
    HIPCHK(hipMemcpyAsync(sh->dRows, x.rows.data(), x.rows.size() * 4, hipMemcpyHostToDevice, sh->stream));
    const int32_t* dSl = nullptr;
    int32_t nTie = 0;
    if (!x.slots.empty()) {
        HIPCHK(hipMemcpyAsync(sh->dSlots, x.slots.data(), x.slots.size() * 4, hipMemcpyHostToDevice, sh->stream));
        dSl = sh->dSlots;
        while (nTie < (int32_t)x.slots.size() && x.slots[nTie] >= 0) ++nTie;
    }
    const bool dense = dense_emulation(pe) && !dSl;
    if (dense && (rc = ensure_xlist(sh))) return rc;
    HIPCHK(hipEventRecord(sh->evA, sh->stream));
    if (nTie > 0) scan_tie_slots(pe, sh, x.slots, nTie);
    launch_emulation(pe, sh, (int32_t)x.rows.size(), dense, dSl, sh->dXdbg);
    HIPCHK(hipGetLastError());
    if (nTie > 0) {
        launch_tie_write(sh->dg, sh->tab, sh->dRows, sh->dSlots, nTie, sh->tie, sh->stream);
        HIPCHK(hipGetLastError());
        st.rowsTieEarly += nTie;
    }
    HIPCHK(hipEventRecord(sh->evB, sh->stream));
    HIPCHK(hipEventSynchronize(sh->evB));
    st.msExactKernel += elapsed(sh->evA, sh->evB);
    st.launchesExact++;
    if (nTie > 0) {
        std::vector<int32_t> redo;
        if ((rc = failed_tie_rows(sh, x.rows.data(), x.slots.data(), nTie, sh->tie.cap, redo)) ||
            (rc = repair_tie_rows(pe, sh, redo, dense)))
            return rc;
        if (!redo.empty()) HIPCHK(hipStreamSynchronize(sh->stream));
    }
    if (sh->dXdbg && pe->hg.n > 10240) print_exact_debug(sh, x.rows, nTie);
    st.rowsExact += (int64_t)x.rows.size();
    return SHD_PE_OK;
}

// One chunk's exact stage.  (dRows: the dense early-stop form overwrites it
// with the exact rows only now, the relax stage's ambiguity bytes being on
// the host.)
static int exact_stage(ShdPe* pe, Shard* sh, const ExactWork& x) {
    if (x.rows.empty()) return SHD_PE_OK;
    if (dense_emulation(pe) && !pe->hg.directed && x.denseIdx.size() == x.rows.size()) {
        const int rc = ensure_tie(pe, sh);
        if (rc) return rc;
        if (sh->tie.cap > 0) return exact_dense_early(pe, sh, x);
    }
    return exact_general(pe, sh, x);
}

// Compute the given table positions (all owned by `sh`), chunked: per chunk
// one relax stage and one exact stage.
static int compute_shard(ShdPe* pe, Shard* sh, const int32_t* pos, int32_t count,
                         BatchTrial* trial = nullptr) {
    if (count <= 0) return SHD_PE_OK;
    sh->pathSrc = -1;               // the exact kernels reuse slot 0
    if (hipSetDevice(sh->device) != hipSuccess) return SHD_PE_EHIP;
    int rc = ensure_table(pe, sh);
    if (rc) return rc;
    ExactWork x;
    ShdPeStats& st = sh->stats;
    HIPCHK(hipEventRecord(sh->ev0, sh->stream));
    for (int32_t c0 = 0; c0 < count; c0 += sh->rowsCap) {
        const int32_t cnt = std::min(sh->rowsCap, count - c0);
        HIPCHK(hipMemcpyAsync(sh->dRows, pos + c0, (size_t)cnt * 4, hipMemcpyHostToDevice,
                              sh->stream));
        x.clear();
        if ((rc = relax_stage(pe, sh, pos + c0, cnt, x, trial)) || (rc = exact_stage(pe, sh, x))) return rc;
    }
    HIPCHK(hipEventRecord(sh->ev1, sh->stream));
    HIPCHK(hipEventSynchronize(sh->ev1));
    st.msTotal += elapsed(sh->ev0, sh->ev1);
    st.rowsComputed += count;
    st.arcsRelaxed += (int64_t)count * pe->hg.nArcs();
    for (int32_t i = 0; i < count; ++i) pe->rowDone[pos[i]].store(1, std::memory_order_release);
    return SHD_PE_OK;
}

Shard* shdpe::owner_of(ShdPe* pe, int32_t p) {
    for (auto& s : pe->shards)
        if (p >= s->rowStart && p < s->rowStart + s->rowCount) return s.get();
    return nullptr;
}

// Compute positions (caller holds pe->mu): split by shard, one host thread
// per shard when several shards have work (their devices run concurrently).
int shdpe::compute_positions_locked(ShdPe* pe, const int32_t* pos, int32_t count) {
    if (count <= 0) return SHD_PE_OK;
    std::vector<std::vector<int32_t>> per(pe->shards.size());
    for (int32_t i = 0; i < count; ++i) {
        Shard* s = owner_of(pe, pos[i]);
        if (!s) return SHD_PE_ENOTOWNED;
        per[s->gindex - pe->firstShard].push_back(pos[i]);
    }
    int busy = 0;
    for (auto& v : per) busy += !v.empty();
    if (busy <= 1) {
        for (size_t k = 0; k < per.size(); ++k)
            if (!per[k].empty()) return compute_shard(pe, pe->shards[k].get(), per[k].data(),
                                                      (int32_t)per[k].size());
        return SHD_PE_OK;
    }
    std::vector<int> rcs(per.size(), SHD_PE_OK);
    std::vector<std::thread> th;
    for (size_t k = 0; k < per.size(); ++k) {
        if (per[k].empty()) continue;
        th.emplace_back([&, k] {
            rcs[k] = compute_shard(pe, pe->shards[k].get(), per[k].data(), (int32_t)per[k].size());
        });
    }
    for (auto& t : th) t.join();
    for (int r : rcs)
        if (r) return r;
    return SHD_PE_OK;
}

bool shdpe::row_done(const ShdPe* pe, int32_t p) {
    return pe->rowDone[p].load(std::memory_order_acquire) != 0;
}

extern "C" int shd_pe_compute_positions(ShdPe* pe, int32_t start, int32_t count) {
    if (!pe || start < 0 || count < 0 || (int64_t)start + count > (int64_t)pe->attached.size())
        return SHD_PE_EINVAL;
    if (count && (start < pe->ownStart || start + count > pe->ownEnd)) return SHD_PE_ENOTOWNED;
    std::vector<int32_t> pos(count);
    for (int32_t i = 0; i < count; ++i) pos[i] = start + i;
    std::lock_guard<std::mutex> lk(pe->mu);
    return compute_positions_locked(pe, pos.data(), count);
}

extern "C" int shd_pe_compute_all(ShdPe* pe) {
    if (!pe) return SHD_PE_EINVAL;
    return shd_pe_compute_positions(pe, pe->ownStart, pe->ownEnd - pe->ownStart);
}

// ---- shd_pe_tune: time the plan's candidates, pick, try a narrower delta ------

// What one candidate's timed compute gave.
struct TuneSample {
    double ms = 0.0;                 // batch kernels in all
    double msRelax = 0.0, msPost = 0.0;   // split kernels: their parts
    int64_t exact = 0;               // rows it sent to the exact path
    // the post kernel in two parts (0 when not timed): the predecessor part,
    // the label part with the redo launch
    double msPred = 0.0, msLabel = 0.0;
};

// The tune's choice among the samples.
struct TunePick {
    int relax = 0, post = 0;         // candidate indices
    int pred = 0, label = 0;         // ... of the post kernel's two parts
    bool split = false;              // the two parts beat the one post kernel
    bool perPart = false;            // picked per part (else one pick for both)
    bool ok[4] = {false, false, false, false};   // candidates that competed
};

// One compute of the shard's rows with the trial's launches.
static int tune_run(ShdPe* pe, Shard* sh, const std::vector<int32_t>& pos, BatchTrial& t, TuneSample& s) {
    const double m0 = sh->stats.msSparseKernel;
    const int64_t x0 = sh->stats.rowsExact;
    t.msRelax = t.msPost = t.msLabel = 0.0;
    const int rc = compute_shard(pe, sh, pos.data(), (int32_t)pos.size(), &t);
    s = TuneSample{sh->stats.msSparseKernel - m0, t.msRelax, t.msPost, sh->stats.rowsExact - x0, 0.0, 0.0};
    if (t.postSplit) {
        s.msPred = t.msPost;
        s.msLabel = t.msLabel;
    } else {
        s.msPost += t.msLabel;      // (one post kernel: the second interval is empty)
    }
    return rc;
}

// Times one candidate as both kernels' variant: a first launch maps its code
// and scratch; the second is timed (split kernels: relax and post separately)
// and, where the shard can run the post kernel in two parts, the same again
// with candidate k as both parts (on the same rows: the comparison the pick
// between one post kernel and two rests on).
static int tune_time(ShdPe* pe, Shard* sh, const std::vector<int32_t>& pos, int k, TuneSample& s) {
    const BatchPlan& plan = sh->plan;
    const BatchLaunch& c = plan.cand[k];
    BatchTrial t;
    t.relax = t.post = c;
    int rc = tune_run(pe, sh, pos, t, s);
    if (rc) return rc;
    t.timed = c.split != 0;
    if ((rc = tune_run(pe, sh, pos, t, s))) return rc;
    if (!c.split || !sh->postSplitOk || pe->tu.postSplit == 0) return SHD_PE_OK;
    BatchTrial u;
    u.relax = u.redo = c;
    u.post = plan.candPred[k];
    u.label = plan.candLabel[k];
    u.postSplit = true;
    TuneSample x;
    if ((rc = tune_run(pe, sh, pos, u, x))) return rc;
    u.timed = true;
    if ((rc = tune_run(pe, sh, pos, u, x))) return rc;
    s.msPred = x.msPred;
    s.msLabel = x.msLabel;
    s.exact = std::max(s.exact, x.exact);
    return SHD_PE_OK;
}

// The picks, from the candidates' samples alone.
static TunePick tune_pick(const BatchLaunch* cand, const TuneSample* s, int nc) {
    TunePick p;
    // Every variant computes the same rows, so they all send the same
    // rows to the exact path -- except one whose batches fail their
    // checks (a miscompiled instantiation: round 6 found one whose post
    // kernel failed every batch's Bellman check under one register
    // allocation).  Such a variant looks FASTER here (its
    // skipped phases are not in the batch-kernel time, the exact kernel
    // is), so it is never picked: only candidates at the fewest exact
    // rows compete.
    int64_t exMin = s[0].exact;
    for (int k = 1; k < nc; ++k) exMin = std::min(exMin, s[k].exact);
    for (int k = 0; k < nc; ++k) p.ok[k] = s[k].exact == exMin;
    // whole launches, or per part when every variant ran split: the
    // relax kernel and the post kernel each take their fastest variant
    p.perPart = true;
    for (int k = 0; k < nc; ++k) p.perPart = p.perPart && cand[k].split && s[k].msRelax > 0.0;
    int rk = 0;
    while (!p.ok[rk]) ++rk;
    int pk = rk;
    for (int k = rk + 1; k < nc; ++k) {
        if (!p.ok[k]) continue;
        if (p.perPart ? s[k].msRelax < s[rk].msRelax : s[k].ms < s[rk].ms) rk = k;
        if (p.perPart ? s[k].msPost < s[pk].msPost : s[k].ms < s[pk].ms) pk = k;
    }
    if (!p.perPart) pk = rk;
    p.relax = rk;
    p.post = pk;
    // the post kernel's two parts, each its fastest variant; taken when their
    // sum beats the fastest one post kernel on these rows
    bool parts = p.perPart;
    for (int k = 0; k < nc; ++k) parts = parts && (!p.ok[k] || (s[k].msPred > 0.0 && s[k].msLabel > 0.0));
    p.pred = p.label = rk;          // (never an excluded candidate, whatever follows)
    if (parts) {
        for (int k = 0; k < nc; ++k) {
            if (!p.ok[k]) continue;
            if (s[k].msPred < s[p.pred].msPred) p.pred = k;
            if (s[k].msLabel < s[p.label].msLabel) p.label = k;
        }
        p.split = s[p.pred].msPred + s[p.label].msLabel < s[pk].msPost;
    }
    return p;
}

// bucket width: the chosen relax variant at delta and at 0.8 x delta,
// timed alternately (A B A B, each width's best run: best[0] at delta,
// best[1] at 0.8 x), the narrower width kept only if its relax kernel is
// faster by more than 1% on this shard -- the gain is 1-2% where it exists
// (C4 same box: N=1 -1.2%, the N=8 shard's LB-8 batches -2%; C5 +1.2%, so
// not a fixed default; profiles/r05_ab_notes.txt r05bg-bi), and a single run
// against a measurement from another pass let noise pick the width.
// The post kernel does not use delta.
static int tune_delta(ShdPe* pe, Shard* sh, const std::vector<int32_t>& pos, BatchLaunch& relax,
                      const BatchLaunch& post, double best[2]) {
    BatchLaunch alt = relax;
    alt.delta = relax.delta * 0.8;
    best[0] = best[1] = 0.0;
    for (int rep = 0; rep < 4; ++rep) {
        BatchTrial t;
        t.relax = (rep & 1) ? alt : relax;
        t.post = post;
        t.timed = true;
        TuneSample s;
        const int rc = tune_run(pe, sh, pos, t, s);
        if (rc) return rc;
        double& b = best[rep & 1];
        if (s.msRelax > 0.0 && (b == 0.0 || s.msRelax < b)) b = s.msRelax;
    }
    if (best[1] > 0.0 && best[0] > 0.0 && best[1] < 0.99 * best[0]) relax = alt;
    return SHD_PE_OK;
}

// Predecessor filter: the post kernel is faster behind a relax variant that
// flags in-arcs (batch_relax_flags: the batch's bits fit in its LDS), so the
// fastest relax alone is not the fastest pair.  When the picked relax does not
// flag and another candidate's does, both pairs (with the picked post
// variant) are timed alternately, A B A B, and the flagging relax is taken if
// its pair's best sum is lower.
static int tune_filter(ShdPe* pe, Shard* sh, const std::vector<int32_t>& pos, const TuneSample* s,
                       TunePick& p) {
    const BatchPlan& plan = sh->plan;
    const int n = pe->hg.n;
    if (!sh->bsc.arcHit || batch_relax_flags(sh->bsc, plan.cand[p.relax], n)) return SHD_PE_OK;
    int fk = -1;
    for (int k = 0; k < plan.nc; ++k)
        if (p.ok[k] && batch_relax_flags(sh->bsc, plan.cand[k], n) && (fk < 0 || s[k].msRelax < s[fk].msRelax))
            fk = k;
    if (fk < 0) return SHD_PE_OK;
    double best[2] = {0.0, 0.0};
    for (int rep = 0; rep < 4; ++rep) {
        BatchTrial t;
        t.relax = plan.cand[(rep & 1) ? fk : p.relax];
        t.post = plan.cand[p.post];
        t.timed = true;
        TuneSample x;
        const int rc = tune_run(pe, sh, pos, t, x);
        if (rc) return rc;
        const double sum = x.msRelax + x.msPost;
        double& b = best[rep & 1];
        if (sum > 0.0 && (b == 0.0 || sum < b)) b = sum;
    }
    if (pe->tu.debug || pe->tu.tuneLog)
        std::fprintf(stderr, "[shdpe] shard %d tune: relax + post %.2f ms behind the %d-wave relax (in-arc flags) vs "
                     "%.2f ms behind the %d-wave relax\n", sh->gindex, best[1], plan.cand[fk].wpe, best[0],
                     plan.cand[p.relax].wpe);
    if (best[1] > 0.0 && best[0] > 0.0 && best[1] < best[0]) p.relax = fk;
    return SHD_PE_OK;
}

static void tune_log(const Shard* sh, const TuneSample* s, const TunePick& p, const double best[2]) {
    const BatchPlan& plan = sh->plan;
    for (int k = 0; k < plan.nc; ++k)
        std::fprintf(stderr, "[shdpe] shard %d tune: %d waves %.2f ms (relax %.2f post %.2f) exact rows %ld%s%s%s\n",
                     sh->gindex, plan.cand[k].wpe, s[k].ms,
                     s[k].msRelax, s[k].msPost, (long)s[k].exact, p.ok[k] ? "" : " (excluded)",
                     k == p.relax ? " <relax" : "", k == p.post ? " <post" : "");
    if (s[p.pred].msPred > 0.0)
        std::fprintf(stderr, "[shdpe] shard %d tune: post kernel %.2f ms (%d waves) vs predecessor part %.2f ms (%d "
                     "waves) + label part %.2f ms (%d waves) -> %s\n", sh->gindex, s[p.post].msPost,
                     plan.cand[p.post].wpe, s[p.pred].msPred, plan.cand[p.pred].wpe, s[p.label].msLabel,
                     plan.cand[p.label].wpe, plan.postSplit ? "two parts" : "one kernel");
    for (int k = 0; k < plan.nc; ++k)
        if (s[k].msPred > 0.0)
            std::fprintf(stderr, "[shdpe] shard %d tune: %d waves as parts: predecessor %.2f ms label %.2f ms\n",
                         sh->gindex, plan.cand[k].wpe, s[k].msPred, s[k].msLabel);
    if (best[1] > 0.0)
        std::fprintf(stderr, "[shdpe] shard %d tune: relax at 0.8 x delta %.2f ms vs %.2f -> delta %.3f\n",
                     sh->gindex, best[1], best[0], plan.relax.delta);
}

// One shard's tune.  Its computes take their launches from trials, so the
// plan changes only when all of them succeeded: a failing compute leaves the
// shard as it was, the untuned picks included.
static int tune_shard(ShdPe* pe, Shard* sh) {
    // scratch first: ensure_batch sizes the slots and lowers the plan's
    // grids to them, and the trials below are copies of those launches
    if (hipSetDevice(sh->device) != hipSuccess) return SHD_PE_EHIP;
    int rc = ensure_table(pe, sh);
    if (!rc) rc = ensure_batch(pe, sh);
    if (rc) return rc;
    BatchPlan& plan = sh->plan;
    std::vector<int32_t> pos(sh->rowCount);
    for (int32_t i = 0; i < sh->rowCount; ++i) pos[i] = sh->rowStart + i;
    const ShdPeStats keep = sh->stats;
    const int64_t keepRedo = sh->redoBatches, keepRounds = sh->roundsRun, keepBatches = sh->batchesRun;
    if (pe->tu.postSplit != 0) (void)ensure_label_arrays(pe, sh);   // (false: only the one post kernel is timed)
    TuneSample s[4];
    for (int k = 0; k < plan.nc && !rc; ++k) rc = tune_time(pe, sh, pos, k, s[k]);
    TunePick p;
    BatchLaunch relax{};
    double best[2] = {0.0, 0.0};
    if (!rc) {
        p = tune_pick(plan.cand, s, plan.nc);
        if (p.perPart) rc = tune_filter(pe, sh, pos, s, p);
        relax = plan.cand[p.relax];
        if (!rc && p.perPart) rc = tune_delta(pe, sh, pos, relax, plan.cand[p.post], best);
    }
    sh->stats = keep;               // the tune's computes are not the caller's
    sh->redoBatches = keepRedo;
    sh->roundsRun = keepRounds;
    sh->batchesRun = keepBatches;
    if (rc) {
        if (!plan.postSplit) release_label_arrays(sh);
        return rc;
    }
    plan.relax = relax;
    plan.redo = p.post != p.relax ? plan.cand[p.post] : relax;
    // (SHDPE_POST_SPLIT=1: the two parts whatever the times say)
    plan.postSplit = sh->postSplitOk && (p.split || (pe->tu.postSplit == 1 && s[p.pred].msPred > 0.0));
    plan.post = plan.postSplit ? plan.candPred[p.pred] : plan.redo;
    if (plan.postSplit) plan.label = plan.candLabel[p.label];
    else release_label_arrays(sh);  // the one post kernel: its labels are per workgroup
    sh->tuned = true;
    plan_stats(pe, sh);
    if (pe->tu.debug || pe->tu.tuneLog) tune_log(sh, s, p, best);
    return SHD_PE_OK;
}

extern "C" int shd_pe_tune(ShdPe* pe) {
    if (!pe) return SHD_PE_EINVAL;
    if (!pe->batched) return SHD_PE_OK;
    std::lock_guard<std::mutex> lk(pe->mu);
    for (auto& sp : pe->shards) {
        Shard* sh = sp.get();
        if (sh->tuned || !sh->plan.tunable() || sh->rowCount <= 0) continue;
        const int rc = tune_shard(pe, sh);
        if (rc) return rc;
    }
    return SHD_PE_OK;
}

extern "C" int shd_pe_compute_rows(ShdPe* pe, const int32_t* src, int32_t count) {
    if (!pe || count < 0 || (count > 0 && !src)) return SHD_PE_EINVAL;
    std::vector<int32_t> pos(count);
    for (int32_t i = 0; i < count; ++i) {
        if (src[i] < 0 || src[i] >= pe->hg.n || pe->posOf[src[i]] < 0) return SHD_PE_ENOTATTACHED;
        pos[i] = pe->posOf[src[i]];
        if (pos[i] < pe->ownStart || pos[i] >= pe->ownEnd) return SHD_PE_ENOTOWNED;
    }
    std::lock_guard<std::mutex> lk(pe->mu);
    return compute_positions_locked(pe, pos.data(), count);
}

// Compute whatever rows of [start, start+count) are owned here and missing.
int shdpe::ensure_rows(ShdPe* pe, int32_t start, int32_t count) {
    bool all = true;
    for (int32_t i = start; i < start + count && all; ++i) all = row_done(pe, i);
    if (all) return SHD_PE_OK;
    std::lock_guard<std::mutex> lk(pe->mu);
    std::vector<int32_t> todo;
    for (int32_t i = start; i < start + count; ++i) {
        if (row_done(pe, i)) continue;
        if (i < pe->ownStart || i >= pe->ownEnd) return SHD_PE_ENOTOWNED;
        todo.push_back(i);
    }
    return compute_positions_locked(pe, todo.data(), (int32_t)todo.size());
}

// The exact kernel for the path code (row i of dRows leaves its parents in scratch slot i;
// dSlots: early-stop rows).  It reuses slot 0: shd_pe_get_path's cached parents do not survive it.
static int paths_emulate(ShdPe* pe, Shard* sh, const int32_t* dRows, int32_t n, int32_t grid,
                         const int32_t* dSlots) {
    sh->pathSrc = -1;
    launch_exact_rows(sh->dg, sh->tab, sh->sc, dRows, n, grid, sh->exactHc, pe->tu.exactHc > 0, dSlots,
                      sh->tie, nullptr, sh->stream);
    HIPCHK(hipGetLastError());
    return SHD_PE_OK;
}

extern "C" int shd_pe_get_path(ShdPe* pe, int32_t srcVertex, int32_t dstVertex, int32_t* verts,
                               int32_t cap, int32_t* len) {
    if (!pe || !verts || !len || cap < 1) return SHD_PE_EINVAL;
    *len = 0;
    const HostGraph& g = pe->hg;
    if (srcVertex < 0 || srcVertex >= g.n || dstVertex < 0 || dstVertex >= g.n) return SHD_PE_EINVAL;
    const int32_t ps = pe->posOf[srcVertex];
    if (ps < 0 || pe->posOf[dstVertex] < 0) return SHD_PE_ENOTATTACHED;
    if (srcVertex == dstVertex) {            // the 1-vertex igraph path [s] (:1469-1488)
        verts[0] = srcVertex;
        *len = 1;
        return SHD_PE_OK;
    }
    if (pe->mode == 2) {                     // complete graph: the direct edge (:1877-1927)
        if (cap < 2) return SHD_PE_EINVAL;
        if (g.findArc(srcVertex, dstVertex) < 0) return SHD_PE_ENOEDGE;
        verts[0] = srcVertex;
        verts[1] = dstVertex;
        *len = 2;
        return SHD_PE_OK;
    }
    std::lock_guard<std::mutex> lk(pe->mu);
    Shard* sh = owner_of(pe, ps);
    if (!sh) return SHD_PE_ENOTOWNED;
    HIPCHK(hipSetDevice(sh->device));
    int rc = ensure_table(pe, sh);
    if (rc) return rc;
    if (!sh->dPath) {
        unsigned char* p;            // in bytes: one PathOne and the n vertices behind it
        if ((rc = dev_alloc(sh, &p, sizeof(PathOne) + (size_t)g.n * 4))) return rc;
        sh->dPath = reinterpret_cast<PathOne*>(p);
    }
    if (sh->pathSrc != srcVertex) {
        // igraph's whole Dijkstra for this source (full 2-wheap emulation,
        // one wave): every vertex popped before the last target keeps its
        // chosen IN-arc in slot 0; the row it rewrites is the table's own
        HIPCHK(hipMemcpyAsync(sh->dRows, &ps, 4, hipMemcpyHostToDevice, sh->stream));
        if ((rc = paths_emulate(pe, sh, sh->dRows, 1, 1, nullptr))) return rc;
        sh->pathSrc = srcVertex;
    }
    // the cell of the row the emulation wrote, judged as k_paths_size judges it: an unreached
    // target has no parent chain in slot 0 (its P entry is whatever an earlier row left there), so
    // it must not be walked; hops gives the length.  (F_NOEDGE: a complete graph's table)
    uint8_t f = 0;
    int32_t hops = 0;
    const size_t cell = (size_t)(ps - sh->tab.rowStart) * pe->attached.size() + pe->posOf[dstVertex];
    HIPCHK(hipMemcpyAsync(&f, sh->tab.flags + cell, 1, hipMemcpyDeviceToHost, sh->stream));
    HIPCHK(hipMemcpyAsync(&hops, sh->tab.hops + cell, 4, hipMemcpyDeviceToHost, sh->stream));
    HIPCHK(hipStreamSynchronize(sh->stream));
    if (f & F_UNREACHABLE) return SHD_PE_EUNREACHABLE;
    if (hops < 1 || hops >= g.n) return SHD_PE_EHIP;
    const int32_t L = hops + 1;
    if (L > cap) return SHD_PE_EINVAL;            // cap too small for the path
    // one request of k_paths_walk over slot 0, in device ids (the batched path relabels vertices)
    const bool relabelled = !pe->devOf.empty();
    PathOne one{0, L, 0, PathReq{0, 0, relabelled ? pe->devOf[srcVertex] : srcVertex,
                                 relabelled ? pe->devOf[dstVertex] : dstVertex}, 0, {}};
    PathOne* const d = sh->dPath;
    int32_t* const dVerts = reinterpret_cast<int32_t*>(d + 1);
    HIPCHK(hipMemcpyAsync(d, &one, sizeof(one), hipMemcpyHostToDevice, sh->stream));
    launch_paths_walk(sh->dg, PathsWalkArgs{&d->req, 1, sh->sc.pred, sh->sc.stride, (int32_t)g.nArcs(), &d->len,
                                            &d->off, dVerts, &d->failed, &d->nFailed}, sh->stream);
    HIPCHK(hipGetLastError());
    std::vector<int32_t> path((size_t)L);
    HIPCHK(hipMemcpyAsync(&one.failed, &d->failed, 1, hipMemcpyDeviceToHost, sh->stream));
    HIPCHK(hipMemcpyAsync(path.data(), dVerts, (size_t)L * 4, hipMemcpyDeviceToHost, sh->stream));
    HIPCHK(hipStreamSynchronize(sh->stream));
    if (one.failed) return SHD_PE_EUNREACHABLE;   // the walk did not arrive at the source
    std::copy(path.begin(), path.end(), verts);
    *len = L;
    return SHD_PE_OK;
}

// ---- shd_pe_get_paths: batched path extraction --------------------
namespace {

constexpr int32_t PATHS_CHUNK = 65536;            // requests per staging chunk
constexpr int64_t PATHS_ENTRIES = (int64_t)1 << 22;   // output entries per chunk (one path may exceed it)
constexpr int32_t PATHS_NOT_MINE = INT32_MIN;     // status preset: another shard answers the request

// Device staging of one shard for one shd_pe_get_paths call (freed with it).
struct PathsStage {
    int device = 0;
    std::vector<void*> mem;
    int32_t *src = nullptr, *dst = nullptr, *posOf = nullptr, *len = nullptr, *stat = nullptr;
    int32_t *verts = nullptr, *nFailed = nullptr;
    int32_t* rows = nullptr;                        // a chunk's unique sources that take the emulation
    int64_t* off = nullptr;
    PathReq *reqs = nullptr, *reqsB = nullptr;      // requests of the emulation tier / of the batch tier
    uint8_t *failed = nullptr, *flags = nullptr;
    double *hopLat = nullptr, *hopRel = nullptr;
    uint64_t *weight = nullptr, *acc = nullptr;     // shd_pe_path_load: the chunk's weights; nArcs + n sums
    uint64_t* issued = nullptr;                     // ... debug counters: global atomic adds issued
    int64_t entries = 0;             // capacity of verts / hopLat / hopRel
    std::vector<int32_t> hLen, hStat;
    std::vector<PathReq> hTrivial, hWalk;   // `reqs` on the host: [trivial | emulation], until the copy-out
    ~PathsStage() {
        if (mem.empty()) return;
        (void)hipSetDevice(device);
        for (void* p : mem) (void)hipFree(p);
    }
    template <class T>
    int get(T** p, size_t count) {
        void* q = nullptr;
        if (hipMalloc(&q, std::max<size_t>(16, count * sizeof(T))) != hipSuccess) return SHD_PE_ENOMEM;
        mem.push_back(q);
        *p = (T*)q;
        return SHD_PE_OK;
    }
};

struct PathsCall {
    const int32_t *src, *dst;
    const ShdPePathsOut* out;
    int32_t chunk;                   // requests per chunk
    int32_t group;                   // sources per emulation group (<= every shard's exactGrid)
    int64_t entries;                 // output entries per chunk
    bool hops;
    const uint64_t* weight = nullptr;    // shd_pe_path_load (out == nullptr): one per request; the chunks'
                                         // paths are reduced into PathsStage::acc, none is copied out
    std::vector<PathsStage> st;      // per local shard
    int64_t c0 = 0;                  // the chunk at hand: requests [c0, c0 + cnt)
    int32_t cnt = 0;
    double ms = 0.0;
};

// The requests of a launch (sorted by slot) whose slot lies in [lo, hi): [first, second).
std::pair<size_t, size_t> reqs_in(const std::vector<PathReq>& reqs, int32_t lo, int32_t hi) {
    const auto below = [](const PathReq& q, int32_t v) { return q.slot < v; };
    const auto a = std::lower_bound(reqs.begin(), reqs.end(), lo, below);
    return {(size_t)(a - reqs.begin()), (size_t)(std::lower_bound(a, reqs.end(), hi, below) - reqs.begin())};
}

// The requests of a chunk that need a parent walk, as one shard answers them:
// what the tiers pass along.  Each tier serves what it can and keeps the rest.
struct PathsWork {
    std::vector<int32_t> uniq;       // the unique sources: table positions in order of first appearance
    std::vector<PathReq> reqs;       // the requests, sorted by the place of their source in uniq; here
                                     // `slot` is that place (a tier's upload carries the slot it walks)

    // from the chunk's requests that shard k answers (hLen > 0), less [s] and,
    // on a complete graph, [s, t]; s / t in device ids
    void build(const ShdPe* pe, const PathsCall& c, size_t k) {
        std::vector<int32_t> place(pe->attached.size(), -1);     // table position -> place in uniq
        const bool relabelled = !pe->devOf.empty();
        for (int32_t i = 0; i < c.cnt && pe->mode != 2; ++i) {
            const int32_t sv = c.src[c.c0 + i], tv = c.dst[c.c0 + i];
            if (c.st[k].hLen[(size_t)i] <= 0 || sv == tv) continue;
            int32_t& p = place[(size_t)pe->posOf[sv]];
            if (p < 0) {
                p = (int32_t)uniq.size();
                uniq.push_back(pe->posOf[sv]);
            }
            reqs.push_back(PathReq{i, p, relabelled ? pe->devOf[sv] : sv, relabelled ? pe->devOf[tv] : tv});
        }
        std::stable_sort(reqs.begin(), reqs.end(),
                         [](const PathReq& a, const PathReq& b) { return a.slot < b.slot; });
    }
    // Keeps the requests i with stay[i] and the sources of those, in order, places renumbered.
    // Returns the number of sources dropped: those whose every request the tier served.
    int64_t keep(const std::vector<uint8_t>& stay) {
        std::vector<int32_t> to(uniq.size(), -1);
        size_t nu = 0, nr = 0;
        for (size_t i = 0; i < reqs.size(); ++i) {
            if (!stay[i]) continue;
            const size_t was = (size_t)reqs[i].slot;             // (>= nu: the places only shrink)
            if (to[was] < 0) {
                to[was] = (int32_t)nu;
                uniq[nu++] = uniq[was];
            }
            reqs[nr] = reqs[i];
            reqs[nr++].slot = to[was];
        }
        reqs.resize(nr);
        uniq.resize(nu);
        return (int64_t)(to.size() - nu);
    }
};

}  // namespace

static int paths_stage_init(ShdPe* pe, PathsCall& c, size_t k) {
    Shard* sh = pe->shards[k].get();
    PathsStage& s = c.st[k];
    if (s.src) return SHD_PE_OK;
    s.device = sh->device;
    int rc;
    const size_t C = (size_t)c.chunk;
    if ((rc = s.get(&s.src, C)) || (rc = s.get(&s.dst, C)) || (rc = s.get(&s.len, C)) ||
        (rc = s.get(&s.stat, C)) || (rc = s.get(&s.off, C + 1)) || (rc = s.get(&s.posOf, (size_t)pe->hg.n)))
        return rc;
    HIPCHK(hipMemcpyAsync(s.posOf, pe->posOf.data(), (size_t)pe->hg.n * 4, hipMemcpyHostToDevice, sh->stream));
    return SHD_PE_OK;
}

// The extraction's part of the staging (not needed by a sizing call).
static int paths_stage_extract(ShdPe* pe, PathsCall& c, size_t k) {
    Shard* sh = pe->shards[k].get();
    PathsStage& s = c.st[k];
    if (s.verts) return SHD_PE_OK;
    int rc;
    const size_t C = (size_t)c.chunk, E = (size_t)c.entries;
    if ((rc = s.get(&s.verts, E)) || (rc = s.get(&s.reqs, C)) || (rc = s.get(&s.reqsB, C)) ||
        (rc = s.get(&s.failed, C)) || (rc = s.get(&s.nFailed, 4)) || (rc = s.get(&s.rows, C)) ||
        (rc = s.get(&s.flags, (size_t)std::min(c.group, sh->rowCount) * pe->attached.size())))
        return rc;
    if (c.hops && ((rc = s.get(&s.hopLat, E)) || (rc = s.get(&s.hopRel, E)))) return rc;
    if (c.weight) {
        const size_t nAcc = (size_t)pe->hg.nArcs() + (size_t)pe->hg.n;
        if ((rc = s.get(&s.weight, C)) || (rc = s.get(&s.acc, nAcc))) return rc;
        HIPCHK(hipMemsetAsync(s.acc, 0, nAcc * 8, sh->stream));
        if (pe->tu.debug) {
            if ((rc = s.get(&s.issued, 1))) return rc;
            HIPCHK(hipMemsetAsync(s.issued, 0, 8, sh->stream));
        }
    }
    s.entries = (int64_t)E;
    return SHD_PE_OK;
}

// Lengths and statuses of requests [c0, c0 + cnt) as shard k answers them
// (hLen / hStat; statuses another shard answers stay PATHS_NOT_MINE), and the
// exclusive scan of its lengths on the device (s.off) for the walk.
static int paths_size_chunk(ShdPe* pe, PathsCall& c, size_t k, int64_t c0, int32_t cnt) {
    Shard* sh = pe->shards[k].get();
    PathsStage& s = c.st[k];
    HIPCHK(hipSetDevice(sh->device));
    int rc = pe->mode == 2 ? SHD_PE_OK : ensure_table(pe, sh);   // (a complete graph's paths need no table)
    if (rc || (rc = paths_stage_init(pe, c, k))) return rc;
    HIPCHK(hipMemcpyAsync(s.src, c.src + c0, (size_t)cnt * 4, hipMemcpyHostToDevice, sh->stream));
    HIPCHK(hipMemcpyAsync(s.dst, c.dst + c0, (size_t)cnt * 4, hipMemcpyHostToDevice, sh->stream));
    HIPCHK(hipEventRecord(sh->ev0, sh->stream));
    HIPCHK(hipMemsetAsync(s.len, 0, (size_t)cnt * 4, sh->stream));
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)s.stat, PATHS_NOT_MINE, (size_t)cnt, sh->stream));
    const PathsSizeArgs a{s.src, s.dst, cnt, s.posOf, pe->ownStart, pe->ownEnd, sh->rowStart,
                          sh->rowStart + sh->rowCount, k == 0 ? 1 : 0, pe->mode == 2 ? 1 : 0, s.len, s.stat};
    launch_paths_size(sh->dgAux, sh->tab, a, sh->stream);
    launch_paths_scan(s.len, cnt, s.off, sh->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(sh->ev1, sh->stream));
    s.hLen.resize((size_t)cnt);
    s.hStat.resize((size_t)cnt);
    HIPCHK(hipMemcpyAsync(s.hLen.data(), s.len, (size_t)cnt * 4, hipMemcpyDeviceToHost, sh->stream));
    HIPCHK(hipMemcpyAsync(s.hStat.data(), s.stat, (size_t)cnt * 4, hipMemcpyDeviceToHost, sh->stream));
    HIPCHK(hipStreamSynchronize(sh->stream));
    c.ms += elapsed(sh->ev0, sh->ev1);
    return SHD_PE_OK;
}

// k_paths_walk over the stage's arrays on the parent arrays at `parents`.
static int paths_walk(const ShdPe* pe, Shard* sh, const PathsStage& s, const PathReq* dReqs, size_t nReqs,
                      const int32_t* parents, int64_t stride, int counter) {
    launch_paths_walk(sh->dg, PathsWalkArgs{dReqs, (int32_t)nReqs, parents, stride, (int32_t)pe->hg.nArcs(),
                                            s.len, s.off, s.verts, s.failed, s.nFailed + counter}, sh->stream);
    HIPCHK(hipGetLastError());
    return SHD_PE_OK;
}

// The requests without a walk: [s] and, on a complete graph, [s, t] (caller's ids).
static int paths_trivial(ShdPe* pe, PathsCall& c, size_t k, PathsWork&) {
    Shard* sh = pe->shards[k].get();
    PathsStage& s = c.st[k];
    s.hTrivial.clear();
    for (int32_t i = 0; i < c.cnt; ++i) {
        const int32_t sv = c.src[c.c0 + i], tv = c.dst[c.c0 + i];
        if (s.hLen[(size_t)i] > 0 && (sv == tv || pe->mode == 2)) s.hTrivial.push_back(PathReq{i, -1, sv, tv});
    }
    if (s.hTrivial.empty()) return SHD_PE_OK;
    HIPCHK(hipMemcpyAsync(s.reqs, s.hTrivial.data(), s.hTrivial.size() * sizeof(PathReq), hipMemcpyHostToDevice,
                          sh->stream));
    return paths_walk(pe, sh, s, s.reqs, s.hTrivial.size(), sh->sc.pred, sh->sc.stride, 0);
}

// Batch tier, on shards that run the split batch kernels (the C4 / C5 default;
// SHDPE_PATHS_FAST=0: off; not sparse, dense, forceMode 3 or latFold): one relax
// + post pass over the work set's sources, and after each round's post kernel
// and tie export one k_paths_walk_dist over the requests whose source sits in
// that round, on the round's persisted distance arrays.  The pass stores no
// table row (BatchTrial::noTable) and ShdPeStats is put back as it was.
// Served: the requests of the rows the pass resolved, less those whose walk
// failed its checks (handed on).  The rows it flagged keep all requests and go
// to `x`: those with a tie slot first (row and slot), then the full emulation's.
static int paths_tier_batch(ShdPe* pe, PathsCall& c, size_t k, PathsWork& w, ExactWork& x) {
    Shard* sh = pe->shards[k].get();
    PathsStage& s = c.st[k];
    int rc;
    if (w.reqs.empty() || !pe->tu.pathsFast || pe->mode != 1 || !pe->batched || pe->opt.forceMode == 3 ||
        pe->hg.latFold || !sh->plan.relax.split)
        return SHD_PE_OK;
    if ((rc = ensure_batch(pe, sh))) return rc;
    if (!sh->plan.relax.split) return SHD_PE_OK;
    BatchTrial trial;   // the plan's picks
    trial.relax = sh->plan.relax;
    trial.post = sh->plan.postSplit ? sh->plan.redo : sh->plan.post;   // (PART 4: the one post kernel)
    trial.noTable = true;
    const int32_t LB = trial.relax.lb;
    // the pass's batch order (table positions, -1 pads); the requests by their source's index in it
    int32_t nB = 0;
    const std::vector<int32_t> order = batch_order(pe->rank, pe->rowOff, LB, w.uniq.data(), (int32_t)w.uniq.size(), nB);
    std::vector<int32_t> ordOf(pe->attached.size());     // by table position
    for (size_t i = 0; i < order.size(); ++i)
        if (order[i] >= 0) ordOf[(size_t)order[i]] = (int32_t)i;
    std::vector<size_t> at(order.size() + 1, 0);         // counting sort: first request of each index
    for (const PathReq& q : w.reqs) ++at[(size_t)ordOf[(size_t)w.uniq[(size_t)q.slot]] + 1];
    for (size_t i = 0; i < order.size(); ++i) at[i + 1] += at[i];
    std::vector<PathReq> breqs(w.reqs.size());
    for (PathReq q : w.reqs) {
        q.slot = ordOf[(size_t)w.uniq[(size_t)q.slot]];
        breqs[at[(size_t)q.slot]++] = q;
    }
    HIPCHK(hipMemcpyAsync(s.reqsB, breqs.data(), breqs.size() * sizeof(PathReq), hipMemcpyHostToDevice, sh->stream));
    const RoundHook walkRound = [&](int32_t r0, int32_t rn) -> int {
        const std::pair<size_t, size_t> r = reqs_in(breqs, r0 * LB, (r0 + rn) * LB);
        const PathsDistArgs a{s.reqsB + r.first, (int32_t)(r.second - r.first), LB, r0 * LB,
                              sh->dBatchAmb + (size_t)r0 * LB, s.len, s.off, s.verts, s.failed};
        launch_paths_walk_dist(sh->dg, sh->bsc, a, sh->stream);
        HIPCHK(hipGetLastError());
        return SHD_PE_OK;
    };
    const ShdPeStats savedStats = sh->stats;
    const int64_t savedRounds[2] = {sh->roundsRun, sh->batchesRun};
    rc = relax_batched(pe, sh, w.uniq.data(), (int32_t)w.uniq.size(), x, &trial, &order, &walkRound);
    sh->stats = savedStats;                              // (relax_batched synchronised: breqs is read)
    sh->roundsRun = savedRounds[0];                      // (shd_pe_batch_info counts the table passes)
    sh->batchesRun = savedRounds[1];
    if (rc) return rc;
    std::vector<uint8_t> failed((size_t)c.cnt), flagged(pe->attached.size(), 0), stay(w.reqs.size());
    HIPCHK(hipMemcpyAsync(failed.data(), s.failed, failed.size(), hipMemcpyDeviceToHost, sh->stream));
    HIPCHK(hipStreamSynchronize(sh->stream));
    HIPCHK(hipMemsetAsync(s.failed, 0, failed.size(), sh->stream));
    for (int32_t p : x.rows) flagged[(size_t)p] = 1;     // (by table position)
    for (size_t i = 0; i < w.reqs.size(); ++i) {
        const bool rowLeft = flagged[(size_t)w.uniq[(size_t)w.reqs[i].slot]];
        stay[i] = rowLeft || failed[(size_t)w.reqs[i].req];
        pe->pathsInfo[3] += stay[i] && !rowLeft;
    }
    pe->pathsInfo[0] += w.keep(stay);
    return SHD_PE_OK;
}

// Tie tier: the early-stop tie rows of the pass (the head of `tie`) run what
// the exact stage runs for them -- relevance scan and the emulation up to the
// row's tie threshold, which leaves the final parents in tie.P of the slot --
// without k_tie_write (the table holds the row already), and one k_paths_walk
// over their requests on tie.P.  Handed on: the rows whose slot failed the
// emulation's consistency check, and the walks that did not arrive.
static int paths_tier_tie(ShdPe* pe, PathsCall& c, size_t k, PathsWork& w, const ExactWork& tie) {
    Shard* sh = pe->shards[k].get();
    PathsStage& s = c.st[k];
    int32_t nTie = 0;
    while (nTie < (int32_t)tie.slots.size() && tie.slots[(size_t)nTie] >= 0) ++nTie;
    if (nTie == 0) return SHD_PE_OK;
    int rc;
    std::vector<int32_t> tieSlot(pe->attached.size(), -1);   // table position -> its tie slot; -2: a bad one
    for (int32_t j = 0; j < nTie; ++j) tieSlot[(size_t)tie.rows[(size_t)j]] = tie.slots[(size_t)j];
    std::vector<PathReq> treqs;
    for (const PathReq& q : w.reqs)
        if (tieSlot[(size_t)w.uniq[(size_t)q.slot]] >= 0)
            treqs.push_back(PathReq{q.req, tieSlot[(size_t)w.uniq[(size_t)q.slot]], q.s, q.t});
    HIPCHK(hipMemcpyAsync(sh->dRows, tie.rows.data(), (size_t)nTie * 4, hipMemcpyHostToDevice, sh->stream));
    HIPCHK(hipMemcpyAsync(sh->dSlots, tie.slots.data(), (size_t)nTie * 4, hipMemcpyHostToDevice, sh->stream));
    HIPCHK(hipMemcpyAsync(s.reqsB, treqs.data(), treqs.size() * sizeof(PathReq), hipMemcpyHostToDevice, sh->stream));
    scan_tie_slots(pe, sh, tie.slots, nTie);
    if ((rc = paths_emulate(pe, sh, sh->dRows, nTie, sh->exactGrid, sh->dSlots)) ||
        (rc = paths_walk(pe, sh, s, s.reqsB, treqs.size(), sh->tie.P, sh->tie.n, 2)))
        return rc;
    std::vector<uint8_t> failed((size_t)c.cnt), stay(w.reqs.size());
    HIPCHK(hipMemcpyAsync(failed.data(), s.failed, failed.size(), hipMemcpyDeviceToHost, sh->stream));
    std::vector<int32_t> redo;                           // (synchronises; treqs is read by then)
    if ((rc = failed_tie_rows(sh, tie.rows.data(), tie.slots.data(), nTie, sh->tie.cap, redo))) return rc;
    HIPCHK(hipMemsetAsync(s.failed, 0, failed.size(), sh->stream));
    for (int32_t p : redo) tieSlot[(size_t)p] = -2;
    for (size_t i = 0; i < w.reqs.size(); ++i) {
        const int32_t sl = tieSlot[(size_t)w.uniq[(size_t)w.reqs[i].slot]];
        stay[i] = sl == -1 || sl == -2 || failed[(size_t)w.reqs[i].req];
        pe->pathsInfo[3] += stay[i] && sl != -1;
    }
    pe->pathsInfo[1] += w.keep(stay);
    return SHD_PE_OK;
}

// Whether shd_pe_get_paths' row tier applies to this engine: switched on
// (shd_pe_paths_set_row_tier), on the per-row sparse kernel or the dense
// min-plus path, the modes whose relax stage the batch tier does not cover.
static bool row_tier_applies(const ShdPe* pe) {
    return pe->pathsRowTier && pe->tu.pathsFast && pe->opt.forceMode != 3 && !pe->hg.latFold &&
           ((pe->mode == 1 && !pe->batched) || pe->mode == 3);
}

// Row tier, sparse form: the work set's sources in groups of at most one row
// per resident workgroup, so k_sparse_rows (the form that stores no table row)
// runs row i of the group in workgroup i and leaves its parents in scratch
// slot i.  Per group: one k_paths_walk over the requests of the rows it did not
// flag; then its tie rows with a slot go through the tie tier's procedure --
// relevance scan, early-stop emulation (enqueued after the walk: it reuses the
// scratch slots), a walk over tie.P, the slots' consistency check.  The slots
// of one group are overwritten by the next.  Handed on: the rows flagged
// without a slot (all their requests), the rows whose slot failed the check,
// and every walk that did not arrive.
static int paths_rows_sparse(ShdPe* pe, PathsCall& c, size_t k, PathsWork& w) {
    Shard* sh = pe->shards[k].get();
    PathsStage& s = c.st[k];
    int rc;
    if ((rc = ensure_tie(pe, sh))) return rc;
    const int32_t G = std::max(1, pe->tu.pathsGroup > 0 ? std::min(pe->tu.pathsGroup, sh->cfg.grid) : sh->cfg.grid);
    const size_t nU = w.uniq.size();
    // per place in uniq: 0 walked on its slot's parents, 1 full emulation, 2 tie slot, 3 a slot that failed
    std::vector<uint8_t> kind(nU, 0), amb((size_t)G);
    std::vector<std::vector<PathReq>> uploads;           // (what the copies read lives until the last
    std::vector<ExactWork> ties;                         // synchronise; growing moves the inner arrays intact)
    sh->pathSrc = -1;                                    // slot 0 is overwritten
    HIPCHK(hipMemcpyAsync(s.rows, w.uniq.data(), nU * 4, hipMemcpyHostToDevice, sh->stream));
    for (size_t u0 = 0; u0 < nU; u0 += (size_t)G) {
        const int32_t g = (int32_t)std::min<size_t>((size_t)G, nU - u0);
        const std::pair<size_t, size_t> r = reqs_in(w.reqs, (int32_t)u0, (int32_t)u0 + g);
        if (sh->dTie) HIPCHK(hipMemsetAsync(sh->tie.count, 0, 4, sh->stream));
        launch_sparse_rows(sh->dg, sh->tab, sh->sc, s.rows + u0, g, sh->dRowAmbig, sh->cfg, nullptr, sh->dTie,
                           sh->stream, true);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(amb.data(), sh->dRowAmbig, (size_t)g, hipMemcpyDeviceToHost, sh->stream));
        HIPCHK(hipStreamSynchronize(sh->stream));
        ties.emplace_back();
        ExactWork& tie = ties.back();                    // the group's tie rows with a slot
        std::vector<int32_t> tiePlace;
        for (int32_t i = 0; i < g; ++i) {
            kind[u0 + (size_t)i] = amb[(size_t)i] >= 2 ? 2 : amb[(size_t)i];
            if (amb[(size_t)i] < 2) continue;
            tie.rows.push_back(w.uniq[u0 + (size_t)i]);
            tie.slots.push_back(amb[(size_t)i] - 2);
            tiePlace.push_back((int32_t)u0 + i);
        }
        uploads.emplace_back();
        std::vector<PathReq>& up = uploads.back();       // [walks on the scratch slots | walks on tie.P]
        for (size_t i = r.first; i < r.second; ++i)
            if (kind[(size_t)w.reqs[i].slot] == 0)
                up.push_back(PathReq{w.reqs[i].req, w.reqs[i].slot - (int32_t)u0, w.reqs[i].s, w.reqs[i].t});
        const size_t nWalk = up.size();
        for (size_t i = r.first; i < r.second; ++i)
            if (kind[(size_t)w.reqs[i].slot] == 2)
                up.push_back(PathReq{w.reqs[i].req, amb[(size_t)w.reqs[i].slot - u0] - 2, w.reqs[i].s, w.reqs[i].t});
        PathReq* const dUp = s.reqsB + r.first;          // (the group's own part of the chunk's requests)
        if (!up.empty())
            HIPCHK(hipMemcpyAsync(dUp, up.data(), up.size() * sizeof(PathReq), hipMemcpyHostToDevice, sh->stream));
        if ((rc = paths_walk(pe, sh, s, dUp, nWalk, sh->sc.pred, sh->sc.stride, 2))) return rc;
        const int32_t nTie = (int32_t)tie.rows.size();
        if (nTie == 0) continue;
        HIPCHK(hipMemcpyAsync(sh->dRows, tie.rows.data(), (size_t)nTie * 4, hipMemcpyHostToDevice, sh->stream));
        HIPCHK(hipMemcpyAsync(sh->dSlots, tie.slots.data(), (size_t)nTie * 4, hipMemcpyHostToDevice, sh->stream));
        scan_tie_slots(pe, sh, tie.slots, nTie);
        if ((rc = paths_emulate(pe, sh, sh->dRows, nTie, sh->exactGrid, sh->dSlots)) ||
            (rc = paths_walk(pe, sh, s, dUp + nWalk, up.size() - nWalk, sh->tie.P, sh->tie.n, 2)))
            return rc;
        std::vector<int32_t> redo;                       // (synchronises)
        if ((rc = failed_tie_rows(sh, tie.rows.data(), tie.slots.data(), nTie, sh->tie.cap, redo))) return rc;
        for (int32_t p : redo)
            for (int32_t j = 0; j < nTie; ++j)
                if (tie.rows[(size_t)j] == p) kind[(size_t)tiePlace[(size_t)j]] = 3;
    }
    std::vector<uint8_t> failed((size_t)c.cnt), stay(w.reqs.size()), left(nU, 0);
    HIPCHK(hipMemcpyAsync(failed.data(), s.failed, failed.size(), hipMemcpyDeviceToHost, sh->stream));
    HIPCHK(hipStreamSynchronize(sh->stream));
    HIPCHK(hipMemsetAsync(s.failed, 0, failed.size(), sh->stream));
    for (size_t i = 0; i < w.reqs.size(); ++i) {
        const size_t pl = (size_t)w.reqs[i].slot;
        stay[i] = kind[pl] == 1 || kind[pl] == 3 || failed[(size_t)w.reqs[i].req];
        pe->pathsInfo[3] += stay[i] && kind[pl] != 1;
        left[pl] |= stay[i];
    }
    for (size_t pl = 0; pl < nU; ++pl)                   // each source served in full, under its tier
        if (!left[pl]) pe->pathsInfo[kind[pl] == 0 ? 6 : 1] += 1;
    w.keep(stay);
    return SHD_PE_OK;
}

// Row tier, dense form: the work set's sources in chunks of the dense batch,
// as relax_dense chunks them; per chunk the min-plus sweeps to convergence
// alone (no predecessor pass, no row writer) and one k_paths_walk_dense over
// the chunk's requests on the converged distance rows, which derives the
// parents along the requested chains only.  A request whose walk meets a tie
// is handed on with its source (no dense tie slots for paths).
static int paths_rows_dense(ShdPe* pe, PathsCall& c, size_t k, PathsWork& w) {
    Shard* sh = pe->shards[k].get();
    PathsStage& s = c.st[k];
    int rc;
    if ((rc = ensure_dense(pe, sh))) return rc;
    const size_t nU = w.uniq.size(), DR = (size_t)sh->denseRows;
    std::vector<PathReq> up = w.reqs;                    // PathReq::slot: the source's row of D in its chunk
    for (PathReq& q : up) q.slot = (int32_t)((size_t)q.slot % DR);
    HIPCHK(hipMemcpyAsync(s.rows, w.uniq.data(), nU * 4, hipMemcpyHostToDevice, sh->stream));
    HIPCHK(hipMemcpyAsync(s.reqsB, up.data(), up.size() * sizeof(PathReq), hipMemcpyHostToDevice, sh->stream));
    for (size_t d0 = 0; d0 < nU; d0 += DR) {
        const int32_t dc = (int32_t)std::min(DR, nU - d0);
        const std::pair<size_t, size_t> r = reqs_in(w.reqs, (int32_t)d0, (int32_t)d0 + dc);
        if (launch_dense_rows(sh->dg, sh->tab, sh->dW, sh->dRl, sh->dD, sh->dP, sh->dRowA, sh->dRowB, sh->dRowAmbD,
                              sh->dAny, sh->dChunkEpoch, s.rows + d0, dc, pe->hg.n, pe->tu, sh->stream, nullptr,
                              nullptr, DENSE_SWEEPS))
            return SHD_PE_EHIP;
        launch_paths_walk_dense(sh->dg, PathsDenseArgs{s.reqsB + r.first, (int32_t)(r.second - r.first), sh->dD,
                                                       (int64_t)pe->hg.n, s.len, s.off, s.verts, s.failed},
                                sh->stream);
        HIPCHK(hipGetLastError());
    }
    std::vector<uint8_t> failed((size_t)c.cnt), stay(w.reqs.size());
    HIPCHK(hipMemcpyAsync(failed.data(), s.failed, failed.size(), hipMemcpyDeviceToHost, sh->stream));
    HIPCHK(hipStreamSynchronize(sh->stream));            // (`up` is read by then)
    HIPCHK(hipMemsetAsync(s.failed, 0, failed.size(), sh->stream));
    for (size_t i = 0; i < w.reqs.size(); ++i) {
        stay[i] = failed[(size_t)w.reqs[i].req];
        pe->pathsInfo[3] += stay[i];
    }
    pe->pathsInfo[6] += w.keep(stay);
    return SHD_PE_OK;
}

// Row tier (shd_pe_paths_set_row_tier; where the batch tier does not apply):
// one pass of the mode's own relax stage over the work set's sources, storing
// no table row, and the walks.  ShdPeStats is put back as it was.
static int paths_tier_rows(ShdPe* pe, PathsCall& c, size_t k, PathsWork& w) {
    Shard* sh = pe->shards[k].get();
    if (w.reqs.empty() || !row_tier_applies(pe)) return SHD_PE_OK;
    const ShdPeStats savedStats = sh->stats;
    const int rc = pe->mode == 3 ? paths_rows_dense(pe, c, k, w) : paths_rows_sparse(pe, c, k, w);
    sh->stats = savedStats;
    return rc;
}

// Grouped emulation, the last tier: igraph's whole Dijkstra for each source
// left, a group per launch: row i of the group runs in workgroup i and leaves
// every popped vertex's chosen IN-arc in scratch slot i (no tie slots: full
// emulations); one k_paths_walk per group.  The emulation rewrites the table
// rows with the same values but marks every entry F_EXACT: the rows' flag
// bytes are saved before and put back after.  (Rows and requests are uploaded
// once, from w.uniq and the stage's hWalk, which stay as they are until the
// chunk's copy-out has synchronised.)
static int paths_tier_emulation(ShdPe* pe, PathsCall& c, size_t k, PathsWork& w) {
    Shard* sh = pe->shards[k].get();
    PathsStage& s = c.st[k];
    if (w.uniq.empty()) return SHD_PE_OK;
    int rc;
    const int32_t G = std::min(c.group, sh->exactGrid);
    s.hWalk = w.reqs;
    for (PathReq& q : s.hWalk) q.slot %= G;
    PathReq* const dWalk = s.reqs + s.hTrivial.size();   // behind the requests without a walk
    HIPCHK(hipMemcpyAsync(s.rows, w.uniq.data(), w.uniq.size() * 4, hipMemcpyHostToDevice, sh->stream));
    HIPCHK(hipMemcpyAsync(dWalk, s.hWalk.data(), s.hWalk.size() * sizeof(PathReq), hipMemcpyHostToDevice,
                          sh->stream));
    for (size_t u0 = 0; u0 < w.uniq.size(); u0 += (size_t)G) {
        const int32_t g = (int32_t)std::min<size_t>((size_t)G, w.uniq.size() - u0);
        const std::pair<size_t, size_t> r = reqs_in(w.reqs, (int32_t)u0, (int32_t)u0 + g);
        launch_paths_flags(sh->tab, s.rows + u0, g, s.flags, false, sh->stream);
        if ((rc = paths_emulate(pe, sh, s.rows + u0, g, g, nullptr))) return rc;
        launch_paths_flags(sh->tab, s.rows + u0, g, s.flags, true, sh->stream);
        HIPCHK(hipGetLastError());
        if ((rc = paths_walk(pe, sh, s, dWalk + r.first, r.second - r.first, sh->sc.pred, sh->sc.stride, 0)))
            return rc;
        pe->pathsInfo[2] += g;
        pe->pathsInfo[4] += 1;
    }
    return SHD_PE_OK;
}

// The hop attributes of the chunk's paths and the copy into the caller's arrays
// at the global offsets.
static int paths_hops_and_copy_out(ShdPe* pe, PathsCall& c, size_t k, int64_t total) {
    Shard* sh = pe->shards[k].get();
    PathsStage& s = c.st[k];
    if (c.hops) {
        launch_paths_hops(sh->dgAux, s.off, c.cnt, total, s.verts, s.hopLat, s.hopRel, s.nFailed + 1, sh->stream);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(sh->ev1, sh->stream));
    int32_t nFailed[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(nFailed, s.nFailed, 8, hipMemcpyDeviceToHost, sh->stream));
    const ShdPePathsOut& o = *c.out;
    const int64_t* goff = o.offsets + c.c0;
    // one shard answers every request: its compact order is the caller's, the
    // DMA lands there; several: through host buffers, path by path
    const bool direct = pe->shards.size() == 1;
    std::vector<int32_t> hv(direct ? 0 : (size_t)total);
    std::vector<double> hl(o.hopLat && !direct ? (size_t)total : 0), hr(o.hopRel && !direct ? (size_t)total : 0);
    HIPCHK(hipMemcpyAsync(direct ? o.verts + goff[0] : hv.data(), s.verts, (size_t)total * 4,
                          hipMemcpyDeviceToHost, sh->stream));
    if (o.hopLat) HIPCHK(hipMemcpyAsync(direct ? o.hopLat + goff[0] : hl.data(), s.hopLat, (size_t)total * 8,
                                        hipMemcpyDeviceToHost, sh->stream));
    if (o.hopRel) HIPCHK(hipMemcpyAsync(direct ? o.hopRel + goff[0] : hr.data(), s.hopRel, (size_t)total * 8,
                                        hipMemcpyDeviceToHost, sh->stream));
    HIPCHK(hipStreamSynchronize(sh->stream));
    if (!direct) {
        int64_t lo = 0;
        for (int32_t i = 0; i < c.cnt; ++i) {
            const int32_t L = s.hLen[(size_t)i];
            if (L <= 0) continue;
            std::memcpy(o.verts + goff[i], hv.data() + lo, (size_t)L * 4);
            if (o.hopLat) std::memcpy(o.hopLat + goff[i], hl.data() + lo, (size_t)L * 8);
            if (o.hopRel) std::memcpy(o.hopRel + goff[i], hr.data() + lo, (size_t)L * 8);
            lo += L;
        }
    }
    c.ms += elapsed(sh->ev0, sh->ev1);
    // the emulation is the last tier: a walk that missed its source, or a hop
    // without an edge, means the scratch parents are not what the table says
    if (nFailed[0] || nFailed[1]) return SHD_PE_EHIP;
    return SHD_PE_OK;
}

// shd_pe_path_load, where paths_hops_and_copy_out stands: the chunk's staged
// paths reduced into the shard's accumulator; only the failure words come back.
static int paths_load_chunk(ShdPe* pe, PathsCall& c, size_t k, int64_t total) {
    Shard* sh = pe->shards[k].get();
    PathsStage& s = c.st[k];
    HIPCHK(hipMemcpyAsync(s.weight, c.weight + c.c0, (size_t)c.cnt * 8, hipMemcpyHostToDevice, sh->stream));
    launch_paths_load(sh->dgAux, PathsLoadArgs{s.off, c.cnt, total, s.verts, s.weight, pe->hg.nArcs(), s.acc,
                                               s.nFailed + 1, pe->tu.loadSlots, s.issued}, sh->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(sh->ev1, sh->stream));
    int32_t nFailed[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(nFailed, s.nFailed, 8, hipMemcpyDeviceToHost, sh->stream));
    HIPCHK(hipStreamSynchronize(sh->stream));
    c.ms += elapsed(sh->ev0, sh->ev1);
    if (nFailed[0] || nFailed[1]) return SHD_PE_EHIP;    // as in paths_hops_and_copy_out
    return SHD_PE_OK;
}

// Paths of the chunk's requests that shard k answers (paths_size_chunk ran):
// the tiers in sequence, then the hop attributes and the copy-out (or, for
// shd_pe_path_load, the reduction).  Each tier serves what it can of the work
// set, counts the sources it served in full into pathsInfo, and leaves in the
// set exactly what it hands on.
static int paths_extract_chunk(ShdPe* pe, PathsCall& c, size_t k) {
    Shard* sh = pe->shards[k].get();
    PathsStage& s = c.st[k];
    int64_t total = 0;
    for (int32_t i = 0; i < c.cnt; ++i) total += s.hLen[(size_t)i];
    if (total == 0) return SHD_PE_OK;
    int rc = paths_stage_extract(pe, c, k);
    if (rc) return rc;
    if (total > s.entries) return SHD_PE_EINVAL;         // (the chunking keeps it within)
    PathsWork w;
    ExactWork tie;                                       // the rows the batch tier's pass flagged
    w.build(pe, c, k);
    HIPCHK(hipEventRecord(sh->ev0, sh->stream));
    HIPCHK(hipMemsetAsync(s.failed, 0, (size_t)c.cnt, sh->stream));
    HIPCHK(hipMemsetAsync(s.nFailed, 0, 16, sh->stream));
    if ((rc = paths_trivial(pe, c, k, w)) || (rc = paths_tier_batch(pe, c, k, w, tie)) ||
        (rc = paths_tier_tie(pe, c, k, w, tie)) || (rc = paths_tier_rows(pe, c, k, w)) ||
        (rc = paths_tier_emulation(pe, c, k, w)))
        return rc;
    return c.weight ? paths_load_chunk(pe, c, k, total) : paths_hops_and_copy_out(pe, c, k, total);
}

// The rows the lengths of these requests are read from, computed first where missing.
static int paths_ensure_rows(ShdPe* pe, const int32_t* src, const int32_t* dst, int64_t count) {
    if (pe->mode == 2) return SHD_PE_OK;
    const HostGraph& g = pe->hg;
    std::vector<int32_t> todo;
    std::vector<uint8_t> seen(pe->attached.size(), 0);
    for (int64_t i = 0; i < count; ++i) {
        const int32_t s = src[i], t = dst[i];
        if (s < 0 || s >= g.n || t < 0 || t >= g.n || s == t) continue;
        const int32_t ps = pe->posOf[s];
        if (ps < pe->ownStart || ps >= pe->ownEnd || pe->posOf[t] < 0 || seen[(size_t)ps]) continue;
        seen[(size_t)ps] = 1;
        if (!row_done(pe, ps)) todo.push_back(ps);
    }
    return compute_positions_locked(pe, todo.data(), (int32_t)todo.size());
}

// The bounds of a call's chunks and groups, and its per-shard staging.
static void paths_call_init(const ShdPe* pe, PathsCall& c, int64_t count) {
    c.chunk = (int32_t)std::min<int64_t>(count, pe->tu.pathsChunk > 0 ? pe->tu.pathsChunk : PATHS_CHUNK);
    c.group = INT32_MAX;
    for (auto& sh : pe->shards) c.group = std::min(c.group, sh->exactGrid);
    // (a chunk's unique sources of a shard fit its dBatchRows / dBatchAmb: they
    // are rows of the shard, so at most min(chunk, rowCount) <= rowsCap)
    c.chunk = std::min(c.chunk, 1 << 20);
    if (pe->tu.pathsGroup > 0) c.group = std::min(c.group, pe->tu.pathsGroup);
    c.entries = std::max<int64_t>(PATHS_ENTRIES, (int64_t)pe->hg.n + 1);
    c.st.resize(pe->shards.size());
}

// Pass 1, sizing: every request's length and status -> offsets (count + 1) and,
// where given, status.
static int paths_size_all(ShdPe* pe, PathsCall& c, int64_t count, int64_t* offsets, int32_t* status) {
    int64_t total = 0;
    offsets[0] = 0;
    for (int64_t c0 = 0; c0 < count; c0 += c.chunk) {
        const int32_t cnt = (int32_t)std::min<int64_t>(c.chunk, count - c0);
        for (size_t k = 0; k < pe->shards.size(); ++k) {
            const int rc = paths_size_chunk(pe, c, k, c0, cnt);
            if (rc) return rc;
        }
        for (int32_t i = 0; i < cnt; ++i) {
            int32_t L = 0, st = SHD_PE_ENOTOWNED;
            for (const PathsStage& s : c.st)
                if (s.hStat[(size_t)i] != PATHS_NOT_MINE) { L = s.hLen[(size_t)i]; st = s.hStat[(size_t)i]; }
            if (status) status[c0 + i] = st;
            total += L;
            offsets[c0 + i + 1] = total;
        }
    }
    return SHD_PE_OK;
}

// Pass 2, extraction: chunks bounded in requests and in output entries.
static int paths_extract_all(ShdPe* pe, PathsCall& c, int64_t count, const int64_t* offsets) {
    for (int64_t c0 = 0; c0 < count;) {
        int64_t c1 = c0 + 1;
        while (c1 < count && c1 - c0 < c.chunk && offsets[c1 + 1] - offsets[c0] <= c.entries) ++c1;
        c.c0 = c0;
        c.cnt = (int32_t)(c1 - c0);
        for (size_t k = 0; k < pe->shards.size(); ++k) {
            int rc;
            if ((rc = paths_size_chunk(pe, c, k, c0, c.cnt)) || (rc = paths_extract_chunk(pe, c, k))) return rc;
        }
        c0 = c1;
    }
    return SHD_PE_OK;
}

extern "C" int shd_pe_get_paths(ShdPe* pe, const int32_t* src, const int32_t* dst, int64_t count,
                                const ShdPePathsOut* out) {
    if (!pe || !out || !out->offsets || count < 0 || (count > 0 && (!src || !dst))) return SHD_PE_EINVAL;
    if (out->verts && out->cap < 0) return SHD_PE_EINVAL;
    if ((out->hopLat || out->hopRel) && !out->verts) return SHD_PE_EINVAL;
    std::lock_guard<std::mutex> lk(pe->mu);
    for (int64_t& x : pe->pathsInfo) x = 0;
    out->offsets[0] = 0;
    if (count == 0) return SHD_PE_OK;
    int rc;
    if ((rc = paths_ensure_rows(pe, src, dst, count))) return rc;
    PathsCall c;
    c.src = src;
    c.dst = dst;
    c.out = out;
    c.hops = out->hopLat || out->hopRel;
    paths_call_init(pe, c, count);
    auto finish = [&](int r) {
        pe->pathsInfo[5] = (int64_t)std::llround(c.ms * 1000.0);
        return r;
    };
    if ((rc = paths_size_all(pe, c, count, out->offsets, out->status))) return finish(rc);
    if (!out->verts) return finish(SHD_PE_OK);
    if (out->offsets[count] > out->cap) return finish(SHD_PE_EINVAL);
    return finish(paths_extract_all(pe, c, count, out->offsets));
}

// shd_pe_get_paths' pipeline up to the end of the tiers, with the requests
// ordered by the table position of their source (SHDPE_LOAD_SORT=0: as given)
// and a reduction in the copy-out's place.  The caller holds pe->mu and has
// zeroed the call's info words; the sums (nArcs + n), the totals and the info
// words are added to (shd_pe_table_load's request route runs this per block of
// sources), status[i] is written where given.
static int path_load_locked(ShdPe* pe, const int32_t* src, const int32_t* dst, const uint64_t* weight,
                            int64_t count, std::vector<uint64_t>& sum, uint64_t tot[4], int32_t* status) {
    const HostGraph& g = pe->hg;
    const size_t nArcs = (size_t)g.nArcs(), nAcc = nArcs + (size_t)g.n;
    std::vector<uint64_t> part, w;                       // one shard's sums; the weights in run order
    std::vector<int64_t> order, offsets;
    std::vector<int32_t> ssrc, sdst, stat;
    if (count == 0) return SHD_PE_OK;
    try {                                                // (every host array of the call: 44 B per request)
        part.resize(nAcc);
        w.resize((size_t)count);
        order.resize((size_t)count);
        offsets.assign((size_t)count + 1, 0);
        ssrc.resize((size_t)count);
        sdst.resize((size_t)count);
        stat.resize((size_t)count);
    } catch (const std::bad_alloc&) {
        return SHD_PE_ENOMEM;
    }
    // a source's pass runs once where its requests share a chunk: by table position, the
    // requests without one (bad ids, unattached) last
    const auto key = [&](int64_t i) {
        const int32_t sv = src[i];
        const int32_t p = sv >= 0 && sv < g.n ? pe->posOf[sv] : -1;
        return p < 0 ? INT32_MAX : p;
    };
    for (int64_t i = 0; i < count; ++i) order[(size_t)i] = i;
    if (pe->tu.loadSort)
        std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return key(a) < key(b); });
    for (int64_t i = 0; i < count; ++i) {
        const int64_t j = order[(size_t)i];
        ssrc[(size_t)i] = src[j];
        sdst[(size_t)i] = dst[j];
        w[(size_t)i] = weight ? weight[j] : 1;
    }
    int rc;
    if ((rc = paths_ensure_rows(pe, ssrc.data(), sdst.data(), count))) return rc;
    PathsCall c;
    c.src = ssrc.data();
    c.dst = sdst.data();
    c.out = nullptr;
    c.hops = false;
    c.weight = w.data();
    paths_call_init(pe, c, count);
    auto finish = [&](int r) {
        pe->pathsInfo[5] += (int64_t)std::llround(c.ms * 1000.0);
        return r;
    };
    if ((rc = paths_size_all(pe, c, count, offsets.data(), stat.data())) ||
        (rc = paths_extract_all(pe, c, count, offsets.data())))
        return finish(rc);
    // the shards' accumulators, summed (integers: in any order)
    for (size_t k = 0; k < pe->shards.size(); ++k) {
        if (!c.st[k].acc) continue;                      // (no request of this shard had a path)
        Shard* sh = pe->shards[k].get();
        HIPCHK(hipSetDevice(sh->device));
        HIPCHK(hipMemcpyAsync(part.data(), c.st[k].acc, nAcc * 8, hipMemcpyDeviceToHost, sh->stream));
        HIPCHK(hipStreamSynchronize(sh->stream));
        for (size_t i = 0; i < nAcc; ++i) sum[i] += part[i];
        if (c.st[k].issued) {
            uint64_t issued = 0;
            HIPCHK(hipMemcpy(&issued, c.st[k].issued, 8, hipMemcpyDeviceToHost));
            pe->loadInfo[1] += (int64_t)issued;
        }
    }
    pe->loadInfo[0] += offsets[(size_t)count];
    for (int64_t i = 0; i < count; ++i) {
        const uint64_t L = (uint64_t)(offsets[(size_t)i + 1] - offsets[(size_t)i]);
        if (status) status[order[(size_t)i]] = stat[(size_t)i];
        if (stat[(size_t)i] != SHD_PE_OK) {
            tot[3] += 1;
            continue;
        }
        tot[0] += 1;
        tot[1] += w[(size_t)i] * L;
        tot[2] += w[(size_t)i] * (L - 1);
    }
    return finish(SHD_PE_OK);
}

// The sums of a load call to the caller's arrays (overwritten, each where given).
static void load_write_out(const ShdPe* pe, const ShdPeLoadOut* out, const std::vector<uint64_t>& sum,
                           const uint64_t tot[4]) {
    const size_t nArcs = (size_t)pe->hg.nArcs();
    if (out->arcLoad) std::memcpy(out->arcLoad, sum.data(), nArcs * 8);
    if (out->vertexLoad) std::memcpy(out->vertexLoad, sum.data() + nArcs, (size_t)pe->hg.n * 8);
    if (out->totals) std::memcpy(out->totals, tot, 32);
}

extern "C" int shd_pe_path_load(ShdPe* pe, const int32_t* src, const int32_t* dst, const uint64_t* weight,
                                int64_t count, const ShdPeLoadOut* out) {
    if (!pe || !out || count < 0 || (count > 0 && (!src || !dst))) return SHD_PE_EINVAL;
    std::lock_guard<std::mutex> lk(pe->mu);
    for (int64_t& x : pe->pathsInfo) x = 0;
    pe->loadInfo[0] = pe->loadInfo[1] = 0;
    uint64_t tot[4] = {0, 0, 0, 0};
    std::vector<uint64_t> sum;
    try {
        sum.assign((size_t)pe->hg.nArcs() + (size_t)pe->hg.n, 0);
    } catch (const std::bad_alloc&) {
        return SHD_PE_ENOMEM;
    }
    const int rc = path_load_locked(pe, src, dst, weight, count, sum, tot, out->status);
    if (rc) return rc;
    load_write_out(pe, out, sum, tot);
    return SHD_PE_OK;
}

// ---- shd_pe_table_load: all-pairs load of a range of source rows --
namespace {

struct PinnedBuf {
    void* p = nullptr;
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    int get(size_t bytes) { return hipHostMalloc(&p, std::max<size_t>(16, bytes), hipHostMallocDefault) == hipSuccess ? SHD_PE_OK : SHD_PE_ENOMEM; }
};
struct OwnedEvent {
    hipEvent_t e = nullptr;
    bool recorded = false;
    ~OwnedEvent() { if (e) (void)hipEventDestroy(e); }
};

// What the tiers of one shd_pe_table_load call add to.
struct TableLoad {
    const ShdPeTableLoadIn* in;
    int64_t T;
    std::vector<uint64_t> sum;           // nArcs + n
    uint64_t tot[4] = {0, 0, 0, 0};
    std::vector<int32_t> rest;           // the table positions left to the request route
    double ms = 0.0;                     // device time of the tree tiers and the direct kernel
    const uint64_t* row(int32_t p) const { return in->weight + (size_t)(p - in->start) * (size_t)in->ld; }
};

constexpr int64_t TLOAD_SCRATCH_BYTES = (int64_t)8 << 30;    // the tree tier's slots, at most
constexpr int64_t TLOAD_BLOCK_REQS = (int64_t)1 << 22;       // requests per block of the request route
constexpr int64_t TLOAD_DIRECT_BYTES = (int64_t)64 << 20;    // weight rows per block of the direct kernel

}  // namespace

// A device accumulator of the call (nArcs + n sums) added into the host's.
static int tload_add_acc(Shard* sh, const uint64_t* dAcc, std::vector<uint64_t>& sum) {
    std::vector<uint64_t> part(sum.size());
    HIPCHK(hipMemcpyAsync(part.data(), dAcc, part.size() * 8, hipMemcpyDeviceToHost, sh->stream));
    HIPCHK(hipStreamSynchronize(sh->stream));
    for (size_t i = 0; i < part.size(); ++i) sum[i] += part[i];
    return SHD_PE_OK;
}

// Direct kernel, complete graphs: every path is the edge (the primary shard, as for shd_pe_get_paths).
static int tload_direct(ShdPe* pe, TableLoad& c) {
    Shard* sh = pe->shards[0].get();
    const ShdPeTableLoadIn* in = c.in;
    const int64_t T = c.T;
    const size_t nAcc = c.sum.size();
    HIPCHK(hipSetDevice(sh->device));
    PathsStage s;
    s.device = sh->device;
    PinnedBuf host;
    OwnedEvent up;
    int32_t* dAtt = nullptr;
    uint64_t *dAcc = nullptr, *dOut = nullptr, *dW = nullptr;
    const int32_t blockRows = (int32_t)std::min<int64_t>({(int64_t)in->count, 65535, std::max<int64_t>(1, TLOAD_DIRECT_BYTES / (8 * T))});
    int rc;
    if ((rc = s.get(&dAtt, (size_t)T)) || (rc = s.get(&dAcc, nAcc)) || (rc = s.get(&dOut, 4))) return rc;
    if (in->weight) {
        if ((rc = s.get(&dW, (size_t)blockRows * (size_t)T)) || (rc = host.get((size_t)blockRows * (size_t)T * 8))) return rc;
        HIPCHK(hipEventCreateWithFlags(&up.e, hipEventDisableTiming));
    }
    HIPCHK(hipMemcpyAsync(dAtt, pe->attached.data(), (size_t)T * 4, hipMemcpyHostToDevice, sh->stream));
    HIPCHK(hipMemsetAsync(dAcc, 0, nAcc * 8, sh->stream));
    HIPCHK(hipMemsetAsync(dOut, 0, 32, sh->stream));
    HIPCHK(hipEventRecord(sh->ev0, sh->stream));
    for (int32_t r0 = 0; r0 < in->count; r0 += blockRows) {
        const int32_t rn = std::min(blockRows, in->count - r0);
        if (in->weight) {
            if (up.recorded) HIPCHK(hipEventSynchronize(up.e));          // the staging is free again
            for (int32_t r = 0; r < rn; ++r)
                std::memcpy((uint64_t*)host.p + (size_t)r * (size_t)T, c.row(in->start + r0 + r), (size_t)T * 8);
            HIPCHK(hipMemcpyAsync(dW, host.p, (size_t)rn * (size_t)T * 8, hipMemcpyHostToDevice, sh->stream));
            HIPCHK(hipEventRecord(up.e, sh->stream));
            up.recorded = true;
        }
        launch_table_direct(sh->dgAux, TableDirectArgs{dAtt, (int32_t)T, in->start + r0, rn, dW, pe->hg.nArcs(), dAcc, dOut},
                            sh->stream);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(sh->ev1, sh->stream));
    uint64_t out[4];
    HIPCHK(hipMemcpyAsync(out, dOut, 32, hipMemcpyDeviceToHost, sh->stream));
    if ((rc = tload_add_acc(sh, dAcc, c.sum))) return rc;
    c.ms += elapsed(sh->ev0, sh->ev1);
    for (int i = 0; i < 4; ++i) c.tot[i] += out[i];
    pe->tloadInfo[1] += in->count;
    return SHD_PE_OK;
}

// ---- parent tier (shd_pe_table_load_set_parent_tier) ----------------
// Where it applies, when switched on: the per-row sparse kernel's engines, the
// tie rows with a slot of the batched engines' tree tier, and the dense mode
// (over the predecessor pass's parent rows, §8i).
static bool tload_parents_apply(const ShdPe* pe) {
    return pe->tloadParentTier && pe->tu.pathsFast && (pe->mode == 1 || pe->mode == 3) && pe->opt.forceMode != 3 &&
           !pe->hg.latFold;
}

namespace {

// One shard's k_tree_load_parents launches of a call: scratch slots, staging
// and what each launch listed (entry e of dHanded is source who[e], launched
// over tie slots where tie[e]).
struct ParentTier {
    PathsStage s;
    PinnedBuf host;
    OwnedEvent up;
    int32_t *dAttDev = nullptr, *dPend = nullptr, *dMark = nullptr;
    uint64_t *dAcc = nullptr, *dOut = nullptr, *dSum = nullptr, *dW = nullptr;
    uint8_t* dHanded = nullptr;
    bool ownAcc = false;
    int grid = 0;
    size_t cap = 0, handedCap = 0;
    std::vector<int32_t> who;
    std::vector<uint8_t> tie;
};

// The parent arrays of one launch: the sparse kernel's scratch slots, the tie
// slots with their thresholds (both in-arc words), or rows of the dense
// predecessor pass's P from row `first` on (vertex ids).
struct ParentRows {
    const int32_t* parents;
    int64_t stride;
    const double* thr;
    bool vertexIds, tie;
};
ParentRows scratch_parents(const Shard* sh) { return {sh->sc.pred, sh->sc.stride, nullptr, false, false}; }
ParentRows tie_parents(const Shard* sh) { return {sh->tie.P, sh->tie.n, sh->tie.thr, false, true}; }
ParentRows dense_parents(const Shard* sh, int64_t n, int64_t first) {
    return {sh->dP + first * n, n, nullptr, true, false};
}

}  // namespace

// cap: sources per launch at most; entries: listed sources of all launches at
// most.  dAcc / dAttDev: the tree tier's, or null (allocated and zeroed here).
static int ptier_init(ShdPe* pe, Shard* sh, const TableLoad& c, size_t cap, size_t entries, uint64_t* dAcc,
                      int32_t* dAttDev, ParentTier& pt) {
    const size_t T = (size_t)c.T, n = (size_t)pe->hg.n, nAcc = c.sum.size();
    int rc;
    pt.s.device = sh->device;
    pt.cap = cap;
    pt.handedCap = entries;
    // scratch slots: one per workgroup, (sum, pending, mark) per vertex
    const int64_t slotBytes = (int64_t)n * 16;
    pt.grid = (int)std::max<size_t>(1, std::min<size_t>((size_t)sh->numCUs, cap));
    pt.grid = (int)std::min<int64_t>(pt.grid, std::max<int64_t>(1, TLOAD_SCRATCH_BYTES / slotBytes));
    if (pe->tu.batchGrid > 0) pt.grid = std::min(pt.grid, pe->tu.batchGrid);
    const size_t slots = (size_t)pt.grid * n;
    if ((rc = pt.s.get(&pt.dOut, 16)) || (rc = pt.s.get(&pt.dHanded, entries)) || (rc = pt.s.get(&pt.dSum, slots)) ||
        (rc = pt.s.get(&pt.dPend, slots)) || (rc = pt.s.get(&pt.dMark, slots)))
        return rc;
    if (c.in->weight) {
        if ((rc = pt.s.get(&pt.dW, cap * T)) || (rc = pt.host.get(cap * T * 8))) return rc;
        HIPCHK(hipEventCreateWithFlags(&pt.up.e, hipEventDisableTiming));
    }
    pt.dAcc = dAcc;
    pt.dAttDev = dAttDev;
    if (!dAcc) {
        pt.ownAcc = true;
        if ((rc = pt.s.get(&pt.dAcc, nAcc)) || (rc = pt.s.get(&pt.dAttDev, T))) return rc;
        std::vector<int32_t> attDev(T);
        for (size_t q = 0; q < T; ++q)
            attDev[q] = pe->devOf.empty() ? pe->attached[q] : pe->devOf[(size_t)pe->attached[q]];
        HIPCHK(hipMemcpy(pt.dAttDev, attDev.data(), T * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemsetAsync(pt.dAcc, 0, nAcc * 8, sh->stream));
    }
    HIPCHK(hipMemsetAsync(pt.dOut, 0, 128, sh->stream));
    HIPCHK(hipMemsetAsync(pt.dHanded, 0, entries, sh->stream));
    return SHD_PE_OK;
}

// One launch over the nSrc <= cap sources at hostPos (dPos: the same on the
// device), their weight rows staged first.  Over the tie slots dSlot with
// their thresholds; else over the arrays 0 .. nSrc - 1 of pr, less dSkip.
static int ptier_launch(ShdPe* pe, Shard* sh, const TableLoad& c, ParentTier& pt, const int32_t* hostPos,
                        int32_t nSrc, const int32_t* dPos, const int32_t* dSlot, const uint8_t* dSkip,
                        const ParentRows& pr) {
    const bool tie = pr.tie;
    const size_t T = (size_t)c.T;
    if (nSrc <= 0) return SHD_PE_OK;
    if ((size_t)nSrc > pt.cap || pt.who.size() + (size_t)nSrc > pt.handedCap) return SHD_PE_EINVAL;
    if (c.in->weight) {
        if (pt.up.recorded) HIPCHK(hipEventSynchronize(pt.up.e));        // the staging is free again
        for (int32_t i = 0; i < nSrc; ++i) std::memcpy((uint64_t*)pt.host.p + (size_t)i * T, c.row(hostPos[i]), T * 8);
        HIPCHK(hipMemcpyAsync(pt.dW, pt.host.p, (size_t)nSrc * T * 8, hipMemcpyHostToDevice, sh->stream));
        HIPCHK(hipEventRecord(pt.up.e, sh->stream));
        pt.up.recorded = true;
    }
    int32_t corruptAt = -1;              // the call's first source (the debug switches' target)
    for (int32_t i = 0; i < nSrc && pe->tu.tloadCorrupt; ++i)
        if (hostPos[i] == c.in->start) corruptAt = i;
    const TreeParentsArgs a{dPos, dSlot, nSrc, pt.dAttDev, pr.parents, pr.stride, (int32_t)pe->hg.nArcs(),
                            pr.vertexIds ? 1 : 0, dSkip, pr.thr, pt.dW, pt.dSum, pt.dPend, pt.dMark,
                            pe->hg.nArcs(), pt.dAcc, pt.dHanded + pt.who.size(), pt.dOut + (tie ? 8 : 0),
                            corruptAt >= 0 ? pe->tu.tloadCorrupt : 0, corruptAt};
    launch_tree_load_parents(sh->dg, sh->dgAux, sh->tab, a, pt.grid, sh->stream);
    HIPCHK(hipGetLastError());
    pt.who.insert(pt.who.end(), hostPos, hostPos + nSrc);
    pt.tie.insert(pt.tie.end(), (size_t)nSrc, (uint8_t)(tie ? 1 : 0));
    return SHD_PE_OK;
}

// The early-stop tie rows rows[0, nTie) with their slots: relevance scan, the
// emulation up to each row's threshold (it leaves the final parents in tie.P),
// and one launch over tie.P.  (rows / slots stay as they are until ptier_finish.)
static int ptier_tie_rows(ShdPe* pe, Shard* sh, const TableLoad& c, ParentTier& pt, const std::vector<int32_t>& rows,
                          const std::vector<int32_t>& slots, int32_t nTie) {
    int rc;
    HIPCHK(hipMemcpyAsync(sh->dRows, rows.data(), (size_t)nTie * 4, hipMemcpyHostToDevice, sh->stream));
    HIPCHK(hipMemcpyAsync(sh->dSlots, slots.data(), (size_t)nTie * 4, hipMemcpyHostToDevice, sh->stream));
    scan_tie_slots(pe, sh, slots, nTie);
    if ((rc = paths_emulate(pe, sh, sh->dRows, nTie, sh->exactGrid, sh->dSlots))) return rc;
    return ptier_launch(pe, sh, c, pt, rows.data(), nTie, sh->dRows, sh->dSlots, nullptr, tie_parents(sh));
}

// Synchronises; the sums (where the accumulator is this tier's own), totals and
// info words of the launches added, handed[e] = listed source e was handed on.
static int ptier_finish(ShdPe* pe, Shard* sh, TableLoad& c, ParentTier& pt, std::vector<uint8_t>& handed) {
    int rc;
    uint64_t out[16];
    handed.assign(pt.who.size(), 0);
    if (!handed.empty())
        HIPCHK(hipMemcpyAsync(handed.data(), pt.dHanded, handed.size(), hipMemcpyDeviceToHost, sh->stream));
    HIPCHK(hipMemcpyAsync(out, pt.dOut, 128, hipMemcpyDeviceToHost, sh->stream));
    if (pt.ownAcc) {
        if ((rc = tload_add_acc(sh, pt.dAcc, c.sum))) return rc;
    } else {
        HIPCHK(hipStreamSynchronize(sh->stream));
    }
    if (out[7] || out[15]) return SHD_PE_EHIP;   // a parent arc the graph does not hold: never
    for (int i = 0; i < 4; ++i) c.tot[i] += out[i] + out[8 + i];
    int64_t nHanded = 0;
    for (uint8_t h : handed) nHanded += h;
    pe->tloadInfo[3] += nHanded;
    pe->tloadInfo[8] += (int64_t)out[4];
    pe->tloadInfo[9] += (int64_t)out[12];
    pe->tloadInfo[10] += (int64_t)(out[5] + out[13]);
    if (pe->tu.debug) pe->tloadInfo[11] += (int64_t)(out[6] + out[14]);
    return SHD_PE_OK;
}

// Parent tier over the table positions [lo, hi) of a shard on the per-row
// sparse kernel: the sources in groups of at most one row per resident
// workgroup, as paths_rows_sparse runs them.  Per group k_sparse_rows in the
// form that stores no table row, one k_tree_load_parents over the scratch slots
// (the rows the kernel flagged skipped by their ambiguity byte), and the
// group's tie rows with a slot through ptier_tie_rows (enqueued after: the
// emulation reuses the scratch slots).  Left to the request route (c.rest):
// the rows flagged for the full emulation and the sources handed on.
static int tload_parents_sparse(ShdPe* pe, size_t k, int32_t lo, int32_t hi, TableLoad& c) {
    Shard* sh = pe->shards[k].get();
    int rc;
    HIPCHK(hipSetDevice(sh->device));
    if ((rc = ensure_table(pe, sh)) || (rc = ensure_tie(pe, sh))) return rc;
    const int32_t count = hi - lo;
    const int32_t G = std::min(count, std::max(1, pe->tu.pathsGroup > 0 ? std::min(pe->tu.pathsGroup, sh->cfg.grid)
                                                                          : sh->cfg.grid));
    ParentTier pt;
    int32_t* dPos = nullptr;
    if ((rc = ptier_init(pe, sh, c, (size_t)G, 2 * (size_t)count, nullptr, nullptr, pt)) ||
        (rc = pt.s.get(&dPos, (size_t)count)))
        return rc;
    std::vector<int32_t> pos((size_t)count);
    for (int32_t p = lo; p < hi; ++p) pos[(size_t)(p - lo)] = p;
    HIPCHK(hipMemcpyAsync(dPos, pos.data(), (size_t)count * 4, hipMemcpyHostToDevice, sh->stream));
    std::vector<uint8_t> amb((size_t)G);
    std::vector<ExactWork> ties;                         // (what the copies read lives until the last synchronise)
    ties.reserve((size_t)((count + G - 1) / G));
    const ShdPeStats savedStats = sh->stats;
    sh->pathSrc = -1;                                    // slot 0 is overwritten
    int64_t nFull = 0;
    const int64_t before = pe->tloadInfo[8] + pe->tloadInfo[9];
    HIPCHK(hipEventRecord(sh->ev0, sh->stream));
    for (int32_t u0 = 0; u0 < count; u0 += G) {
        const int32_t g = std::min(G, count - u0);
        if (sh->dTie) HIPCHK(hipMemsetAsync(sh->tie.count, 0, 4, sh->stream));
        launch_sparse_rows(sh->dg, sh->tab, sh->sc, dPos + u0, g, sh->dRowAmbig, sh->cfg, nullptr, sh->dTie,
                           sh->stream, true);
        HIPCHK(hipGetLastError());
        if ((rc = ptier_launch(pe, sh, c, pt, pos.data() + u0, g, dPos + u0, nullptr, sh->dRowAmbig, scratch_parents(sh))))
            return rc;
        HIPCHK(hipMemcpyAsync(amb.data(), sh->dRowAmbig, (size_t)g, hipMemcpyDeviceToHost, sh->stream));
        HIPCHK(hipStreamSynchronize(sh->stream));
        ties.emplace_back();
        ExactWork& tie = ties.back();                    // the group's tie rows with a slot
        for (int32_t i = 0; i < g; ++i) {
            if (amb[(size_t)i] == 1) {
                c.rest.push_back(pos[(size_t)(u0 + i)]);
                ++nFull;
            } else if (amb[(size_t)i] >= 2) {
                tie.rows.push_back(pos[(size_t)(u0 + i)]);
                tie.slots.push_back(amb[(size_t)i] - 2);
            }
        }
        if (!tie.rows.empty() &&
            (rc = ptier_tie_rows(pe, sh, c, pt, tie.rows, tie.slots, (int32_t)tie.rows.size())))
            return rc;
    }
    HIPCHK(hipEventRecord(sh->ev1, sh->stream));
    std::vector<uint8_t> handed;
    rc = ptier_finish(pe, sh, c, pt, handed);
    sh->stats = savedStats;
    if (rc) return rc;
    c.ms += elapsed(sh->ev0, sh->ev1);
    int64_t nHanded = 0;
    for (size_t e = 0; e < handed.size(); ++e)
        if (handed[e]) {
            c.rest.push_back(pt.who[e]);
            ++nHanded;
        }
    if (pe->tloadInfo[8] + pe->tloadInfo[9] - before + nHanded + nFull != (int64_t)count) return SHD_PE_EHIP;
    return SHD_PE_OK;
}

// Parent tier over the table positions [lo, hi) of a shard in the dense mode
// (§8i): the positions in chunks of the dense batch, as relax_dense chunks
// them.  Per chunk the sweeps and the predecessor pass without the row writer
// (DENSE_PRED), then k_tree_load_parents over the chunk's rows of P (vertex
// ids; the rows with a tie skipped by their rowAmb byte), launched in blocks of
// sources whose weight rows stay within TLOAD_DIRECT_BYTES of staging.  The
// chunk's tie rows, on an undirected graph with tie slots: exported while D / P
// hold them, the relevance scan, k_exact_dense's early stop -- the table's own
// dense exact stage without k_tie_write -- and the kernel over tie.P (in-arc
// words).  Left to the request route (c.rest): a chunk's tie rows beyond the
// slots, every tie row of a directed graph, and the sources handed on.
static int tload_parents_dense(ShdPe* pe, size_t k, int32_t lo, int32_t hi, TableLoad& c) {
    Shard* sh = pe->shards[k].get();
    int rc;
    HIPCHK(hipSetDevice(sh->device));
    if ((rc = ensure_table(pe, sh)) || (rc = ensure_dense(pe, sh)) || (rc = ensure_tie(pe, sh))) return rc;
    const int32_t count = hi - lo, DR = sh->denseRows;
    const int64_t n = pe->hg.n;
    const int32_t slotCap = sh->dTie && !pe->hg.directed ? sh->tie.cap : 0;
    const int32_t block = (int32_t)std::min<int64_t>(count, std::max<int64_t>(1, TLOAD_DIRECT_BYTES / (8 * c.T)));
    if (slotCap > 0) {
        if (!sh->dDenseIdx && (rc = dev_alloc(sh, &sh->dDenseIdx, (size_t)sh->rowsCap))) return rc;
        if ((rc = ensure_xlist(sh))) return rc;
    }
    ParentTier pt;
    int32_t* dPos = nullptr;
    if ((rc = ptier_init(pe, sh, c, (size_t)block, 2 * (size_t)count, nullptr, nullptr, pt)) ||
        (rc = pt.s.get(&dPos, (size_t)count)))
        return rc;
    std::vector<int32_t> pos((size_t)count), slots((size_t)slotCap);
    for (int32_t p = lo; p < hi; ++p) pos[(size_t)(p - lo)] = p;
    for (int32_t i = 0; i < slotCap; ++i) slots[(size_t)i] = i;
    HIPCHK(hipMemcpyAsync(dPos, pos.data(), (size_t)count * 4, hipMemcpyHostToDevice, sh->stream));
    if (slotCap > 0)
        HIPCHK(hipMemcpyAsync(sh->dSlots, slots.data(), (size_t)slotCap * 4, hipMemcpyHostToDevice, sh->stream));
    std::vector<uint8_t> amb;
    std::vector<ExactWork> ties;                         // (what the copies read lives until the last synchronise)
    ties.reserve((size_t)((count + DR - 1) / DR));
    const ShdPeStats savedStats = sh->stats;
    int64_t nRest = 0;
    const int64_t before = pe->tloadInfo[8] + pe->tloadInfo[9];
    HIPCHK(hipEventRecord(sh->ev0, sh->stream));
    for (int32_t d0 = 0; d0 < count; d0 += DR) {
        const int32_t dc = std::min(DR, count - d0);
        if (launch_dense_rows(sh->dg, sh->tab, sh->dW, sh->dRl, sh->dD, sh->dP, sh->dRowA, sh->dRowB, sh->dRowAmbD,
                              sh->dAny, sh->dChunkEpoch, dPos + d0, dc, n, pe->tu, sh->stream, nullptr, nullptr,
                              DENSE_PRED))
            return SHD_PE_EHIP;
        HIPCHK(hipGetLastError());
        amb.resize((size_t)dc);
        HIPCHK(hipMemcpyAsync(amb.data(), sh->dRowAmbD, (size_t)dc, hipMemcpyDeviceToHost, sh->stream));
        for (int32_t b0 = 0; b0 < dc; b0 += block)
            if ((rc = ptier_launch(pe, sh, c, pt, pos.data() + d0 + b0, std::min(block, dc - b0), dPos + d0 + b0, nullptr,
                                   sh->dRowAmbD + b0, dense_parents(sh, n, b0))))
                return rc;
        HIPCHK(hipStreamSynchronize(sh->stream));
        ties.emplace_back();
        ExactWork& tie = ties.back();                    // the chunk's tie rows with a slot
        for (int32_t i = 0; i < dc; ++i) {
            if (!amb[(size_t)i]) continue;
            if ((int32_t)tie.rows.size() < slotCap) {
                tie.rows.push_back(pos[(size_t)(d0 + i)]);
                tie.denseIdx.push_back(i);
            } else {
                c.rest.push_back(pos[(size_t)(d0 + i)]);
                ++nRest;
            }
        }
        const int32_t nTie = (int32_t)tie.rows.size();
        if (nTie == 0) continue;
        sh->pathSrc = -1;                                // the emulation overwrites slot 0
        HIPCHK(hipMemcpyAsync(sh->dRows, tie.rows.data(), (size_t)nTie * 4, hipMemcpyHostToDevice, sh->stream));
        HIPCHK(hipMemcpyAsync(sh->dDenseIdx, tie.denseIdx.data(), (size_t)nTie * 4, hipMemcpyHostToDevice, sh->stream));
        HIPCHK(hipMemsetAsync(sh->tie.thr, 0, (size_t)nTie * 8, sh->stream));
        launch_dense_tie_export(sh->dg, sh->dD, sh->dP, n, sh->dDenseIdx, sh->dRows, sh->tie, nTie, sh->stream);
        scan_tie_slots(pe, sh, slots, nTie);
        HIPCHK(hipMemsetAsync(sh->tie.count + 2, 0, 4, sh->stream));
        launch_exact_dense(sh->dg, sh->tab, sh->sc, sh->dRows, nTie, sh->exactGrid, sh->exactHc, sh->dXList,
                           sh->dSlots, sh->tie, sh->tie.count + 2, sh->stream);
        HIPCHK(hipGetLastError());
        for (int32_t b0 = 0; b0 < nTie; b0 += block)
            if ((rc = ptier_launch(pe, sh, c, pt, tie.rows.data() + b0, std::min(block, nTie - b0), sh->dRows + b0,
                                   sh->dSlots + b0, nullptr, tie_parents(sh))))
                return rc;
    }
    HIPCHK(hipEventRecord(sh->ev1, sh->stream));
    std::vector<uint8_t> handed;
    rc = ptier_finish(pe, sh, c, pt, handed);
    sh->stats = savedStats;
    if (rc) return rc;
    c.ms += elapsed(sh->ev0, sh->ev1);
    int64_t nHanded = 0;
    for (size_t e = 0; e < handed.size(); ++e)
        if (handed[e]) {
            c.rest.push_back(pt.who[e]);
            ++nHanded;
        }
    if (pe->tloadInfo[8] + pe->tloadInfo[9] - before + nHanded + nRest != (int64_t)count) return SHD_PE_EHIP;
    return SHD_PE_OK;
}

// Where paths_tier_batch applies (the split batch kernels), and the tier is on.
static bool tload_tree_applies(const ShdPe* pe) {
    return pe->tu.tloadTree && pe->tu.pathsFast && pe->mode == 1 && pe->batched && pe->opt.forceMode != 3 &&
           !pe->hg.latFold;
}

// Tree tier over the table positions [lo, hi) of shard k: one pass of the split
// kernels that stores no row, as paths_tier_batch runs it, and after each
// round's post kernel and tie export one k_tree_load over the round's batches.
// The round's weight rows go up through page-locked staging while its relax
// runs.  Left to the request route (c.rest): the rows the pass flagged and the
// sources the kernel handed on.
static int tload_tree_shard(ShdPe* pe, size_t k, int32_t lo, int32_t hi, TableLoad& c) {
    Shard* sh = pe->shards[k].get();
    const ShdPeTableLoadIn* in = c.in;
    const size_t T = (size_t)c.T, nAcc = c.sum.size(), n = (size_t)pe->hg.n;
    int rc;
    auto all_rest = [&]() {
        for (int32_t p = lo; p < hi; ++p) c.rest.push_back(p);
        return SHD_PE_OK;
    };
    HIPCHK(hipSetDevice(sh->device));
    if (!sh->plan.relax.split) return all_rest();
    if ((rc = ensure_table(pe, sh)) || (rc = ensure_batch(pe, sh))) return rc;
    if (!sh->plan.relax.split) return all_rest();
    BatchTrial trial;   // the plan's picks, as paths_tier_batch
    trial.relax = sh->plan.relax;
    trial.post = sh->plan.postSplit ? sh->plan.redo : sh->plan.post;
    trial.noTable = true;
    const int32_t LB = trial.relax.lb;
    std::vector<int32_t> pos((size_t)(hi - lo));
    for (int32_t p = lo; p < hi; ++p) pos[(size_t)(p - lo)] = p;
    int32_t nB = 0;
    const std::vector<int32_t> order = batch_order(pe->rank, pe->rowOff, LB, pos.data(), (int32_t)pos.size(), nB);
    const int32_t roundCap = std::min(sh->batchRound, nB);
    int64_t firstAt = -1;                // the call's first source in `order` (the debug switches' target)
    for (size_t i = 0; i < order.size() && pe->tu.tloadCorrupt; ++i)
        if (order[i] == in->start) firstAt = (int64_t)i;
    // scratch slots: one per workgroup, (parent, sum, pending) per (vertex, lane)
    const int64_t slotBytes = (int64_t)n * LB * 16;
    int grid = std::max(1, std::min<int>(sh->numCUs, roundCap));
    grid = (int)std::min<int64_t>(grid, std::max<int64_t>(1, TLOAD_SCRATCH_BYTES / slotBytes));
    if (pe->tu.batchGrid > 0) grid = std::min(grid, pe->tu.batchGrid);
    PathsStage s;
    s.device = sh->device;
    PinnedBuf host;
    OwnedEvent up;
    int32_t *dAttDev = nullptr, *dPar = nullptr, *dPend = nullptr;
    uint64_t *dAcc = nullptr, *dOut = nullptr, *dSum = nullptr, *dW = nullptr;
    uint8_t* dHanded = nullptr;
    const size_t slotEntries = (size_t)grid * n * (size_t)LB, roundW = (size_t)roundCap * (size_t)LB * T;
    if ((rc = s.get(&dAttDev, T)) || (rc = s.get(&dAcc, nAcc)) || (rc = s.get(&dOut, 8)) ||
        (rc = s.get(&dHanded, order.size())) || (rc = s.get(&dPar, slotEntries)) || (rc = s.get(&dSum, slotEntries)) ||
        (rc = s.get(&dPend, slotEntries)))
        return rc;
    if (in->weight) {
        if ((rc = s.get(&dW, roundW)) || (rc = host.get(roundW * 8))) return rc;
        HIPCHK(hipEventCreateWithFlags(&up.e, hipEventDisableTiming));
    }
    std::vector<int32_t> attDev(T);
    for (size_t q = 0; q < T; ++q) attDev[q] = pe->devOf.empty() ? pe->attached[q] : pe->devOf[(size_t)pe->attached[q]];
    HIPCHK(hipMemcpyAsync(dAttDev, attDev.data(), T * 4, hipMemcpyHostToDevice, sh->stream));
    HIPCHK(hipMemsetAsync(dAcc, 0, nAcc * 8, sh->stream));
    HIPCHK(hipMemsetAsync(dOut, 0, 64, sh->stream));
    HIPCHK(hipMemsetAsync(dHanded, 0, order.size(), sh->stream));
    int64_t rounds = 0;
    const RoundHook treeRound = [&](int32_t r0, int32_t rn) -> int {
        const size_t ro = (size_t)r0 * LB, cnt = (size_t)rn * LB;
        if (in->weight) {
            if (up.recorded) HIPCHK(hipEventSynchronize(up.e));          // the staging is free again
            for (size_t i = 0; i < cnt; ++i)
                if (order[ro + i] >= 0) std::memcpy((uint64_t*)host.p + i * T, c.row(order[ro + i]), T * 8);
            HIPCHK(hipMemcpyAsync(dW, host.p, cnt * T * 8, hipMemcpyHostToDevice, sh->stream));
            HIPCHK(hipEventRecord(up.e, sh->stream));
            up.recorded = true;
        }
        const bool here = firstAt >= (int64_t)ro && firstAt < (int64_t)(ro + cnt);
        const TreeLoadArgs a{sh->dBatchRows + ro, sh->dBatchAmb + ro, rn, LB, dAttDev, dW, dPar, dSum, dPend,
                             pe->hg.nArcs(), dAcc, dHanded + ro, dOut, here ? pe->tu.tloadCorrupt : 0,
                             here ? (int32_t)(firstAt - (int64_t)ro) : -1};
        launch_tree_load(sh->dg, sh->dgAux, sh->tab, sh->bsc, a, grid, sh->stream);
        HIPCHK(hipGetLastError());
        ++rounds;
        return SHD_PE_OK;
    };
    ExactWork x;
    const ShdPeStats savedStats = sh->stats;
    const int64_t savedRounds[2] = {sh->roundsRun, sh->batchesRun};
    HIPCHK(hipEventRecord(sh->ev0, sh->stream));
    rc = relax_batched(pe, sh, pos.data(), (int32_t)pos.size(), x, &trial, &order, &treeRound);
    sh->stats = savedStats;
    sh->roundsRun = savedRounds[0];
    sh->batchesRun = savedRounds[1];
    if (rc) return rc;
    // parent tier: the flagged rows with a tie slot (the head of x) over the slots' final parents
    ParentTier pt;
    int32_t nTie = 0;
    while (tload_parents_apply(pe) && nTie < (int32_t)x.slots.size() && x.slots[(size_t)nTie] >= 0) ++nTie;
    if (nTie > 0 && ((rc = ptier_init(pe, sh, c, (size_t)nTie, (size_t)nTie, dAcc, dAttDev, pt)) ||
                     (rc = ptier_tie_rows(pe, sh, c, pt, x.rows, x.slots, nTie))))
        return rc;
    HIPCHK(hipEventRecord(sh->ev1, sh->stream));
    std::vector<uint8_t> handed(order.size());
    uint64_t out[8];
    HIPCHK(hipMemcpyAsync(handed.data(), dHanded, handed.size(), hipMemcpyDeviceToHost, sh->stream));
    HIPCHK(hipMemcpyAsync(out, dOut, 64, hipMemcpyDeviceToHost, sh->stream));
    if ((rc = tload_add_acc(sh, dAcc, c.sum))) return rc;
    c.ms += elapsed(sh->ev0, sh->ev1);
    if (out[7]) return SHD_PE_EHIP;      // a parent arc the graph does not hold: never
    for (int i = 0; i < 4; ++i) c.tot[i] += out[i];
    int64_t nHanded = 0, nTieServed = 0;
    std::vector<uint8_t> tieHanded;      // (x.rows[j], j < nTie: handed on by the parent tier)
    if (nTie > 0) {
        const int64_t before = pe->tloadInfo[9];
        if ((rc = ptier_finish(pe, sh, c, pt, tieHanded))) return rc;
        nTieServed = pe->tloadInfo[9] - before;
    }
    for (size_t j = 0; j < x.rows.size(); ++j)
        if (j >= (size_t)nTie || tieHanded[j]) c.rest.push_back(x.rows[j]);
    for (size_t i = 0; i < order.size(); ++i)
        if (order[i] >= 0 && handed[i]) {
            c.rest.push_back(order[i]);
            ++nHanded;
        }
    if (nTieServed + (int64_t)std::count(tieHanded.begin(), tieHanded.end(), 1) != nTie) return SHD_PE_EHIP;
    if ((int64_t)out[4] + nHanded + (int64_t)x.rows.size() != (int64_t)pos.size()) return SHD_PE_EHIP;
    pe->tloadInfo[0] += (int64_t)out[4];
    pe->tloadInfo[3] += nHanded;
    pe->tloadInfo[4] += (int64_t)out[5];
    pe->tloadInfo[6] += rounds;
    if (pe->tu.debug) pe->tloadInfo[7] += (int64_t)out[6];
    return SHD_PE_OK;
}

// Request route: shd_pe_path_load's pipeline on the pairs of the sources left,
// made here block by block, source-major (so its sort by source moves nothing).
static int tload_route(ShdPe* pe, TableLoad& c) {
    const ShdPeTableLoadIn* in = c.in;
    const int64_t T = c.T;
    std::sort(c.rest.begin(), c.rest.end());
    const size_t per = (size_t)std::max<int64_t>(1, TLOAD_BLOCK_REQS / T);
    std::vector<int32_t> src, dst;
    std::vector<uint64_t> w;
    for (size_t b0 = 0; b0 < c.rest.size(); b0 += per) {
        const size_t bn = std::min(per, c.rest.size() - b0);
        try {
            src.resize(bn * (size_t)T);
            dst.resize(bn * (size_t)T);
            if (in->weight) w.resize(bn * (size_t)T);
        } catch (const std::bad_alloc&) {
            return SHD_PE_ENOMEM;
        }
        for (size_t i = 0; i < bn; ++i) {
            const int32_t p = c.rest[b0 + i];
            std::fill_n(src.begin() + (ptrdiff_t)(i * (size_t)T), (size_t)T, pe->attached[(size_t)p]);
            std::copy(pe->attached.begin(), pe->attached.end(), dst.begin() + (ptrdiff_t)(i * (size_t)T));
            if (in->weight) std::memcpy(w.data() + i * (size_t)T, c.row(p), (size_t)T * 8);
        }
        const int rc = path_load_locked(pe, src.data(), dst.data(), in->weight ? w.data() : nullptr,
                                        (int64_t)(bn * (size_t)T), c.sum, c.tot, nullptr);
        if (rc) return rc;
        pe->tloadInfo[2] += (int64_t)bn;
    }
    return SHD_PE_OK;
}

extern "C" int shd_pe_table_load(ShdPe* pe, const ShdPeTableLoadIn* in, const ShdPeLoadOut* out) {
    if (!pe || !in || !out) return SHD_PE_EINVAL;
    const int64_t T = (int64_t)pe->attached.size();
    if (in->start < 0 || in->count < 0 || (int64_t)in->start + in->count > T) return SHD_PE_EINVAL;
    if (in->weight && in->ld < T) return SHD_PE_EINVAL;
    std::lock_guard<std::mutex> lk(pe->mu);
    const int32_t lo = in->start, hi = in->start + in->count;
    if (in->count > 0 && pe->mode != 2 && pe->opt.shardCount > 1 && !pe->gathered &&
        (lo < pe->ownStart || hi > pe->ownEnd))
        return SHD_PE_ENOTOWNED;
    for (int64_t& x : pe->pathsInfo) x = 0;
    for (int64_t& x : pe->tloadInfo) x = 0;
    pe->loadInfo[0] = pe->loadInfo[1] = 0;
    TableLoad c;
    c.in = in;
    c.T = T;
    try {
        c.sum.assign((size_t)pe->hg.nArcs() + (size_t)pe->hg.n, 0);
    } catch (const std::bad_alloc&) {
        return SHD_PE_ENOMEM;
    }
    int rc = SHD_PE_OK;
    if (in->count > 0 && pe->mode == 2) {
        rc = tload_direct(pe, c);
    } else if (in->count > 0) {
        std::vector<int32_t> todo;       // rows not yet computed: first
        for (int32_t p = std::max(lo, pe->ownStart); p < std::min(hi, pe->ownEnd); ++p)
            if (!row_done(pe, p)) todo.push_back(p);
        if ((rc = compute_positions_locked(pe, todo.data(), (int32_t)todo.size()))) return rc;
        std::vector<uint8_t> seen((size_t)in->count, 0);
        for (size_t k = 0; k < pe->shards.size() && tload_tree_applies(pe); ++k) {
            const Shard* sh = pe->shards[k].get();
            const int32_t a = std::max(lo, sh->rowStart), b = std::min(hi, sh->rowStart + sh->rowCount);
            if (a >= b) continue;
            if ((rc = tload_tree_shard(pe, k, a, b, c))) return rc;
            std::fill(seen.begin() + (a - lo), seen.begin() + (b - lo), (uint8_t)1);
        }
        for (size_t k = 0; k < pe->shards.size() && tload_parents_apply(pe) && !pe->batched; ++k) {
            const Shard* sh = pe->shards[k].get();
            const int32_t a = std::max(lo, sh->rowStart), b = std::min(hi, sh->rowStart + sh->rowCount);
            if (a >= b) continue;
            if ((rc = pe->mode == 3 ? tload_parents_dense(pe, k, a, b, c) : tload_parents_sparse(pe, k, a, b, c)))
                return rc;
            std::fill(seen.begin() + (a - lo), seen.begin() + (b - lo), (uint8_t)1);
        }
        for (int32_t p = lo; p < hi; ++p)
            if (!seen[(size_t)(p - lo)]) c.rest.push_back(p);
        rc = tload_route(pe, c);
    }
    if (rc) return rc;
    pe->tloadInfo[5] = (int64_t)std::llround(c.ms * 1000.0) + pe->pathsInfo[5];
    load_write_out(pe, out, c.sum, c.tot);
    return SHD_PE_OK;
}

extern "C" int shd_pe_table_load_info(const ShdPe* pe, int64_t* info, int32_t n) {
    if (!pe || !info || n < 0) return SHD_PE_EINVAL;
    std::lock_guard<std::mutex> lk(const_cast<ShdPe*>(pe)->mu);
    for (int32_t k = 0; k < std::min<int32_t>(n, 12); ++k) info[k] = pe->tloadInfo[k];
    return SHD_PE_OK;
}

extern "C" int shd_pe_table_load_set_parent_tier(ShdPe* pe, int32_t enable) {
    if (!pe) return SHD_PE_EINVAL;
    std::lock_guard<std::mutex> lk(pe->mu);
    pe->tloadParentTier = enable != 0;
    return SHD_PE_OK;
}

extern "C" int shd_pe_path_load_info(const ShdPe* pe, int64_t* info, int32_t n) {
    if (!pe || !info || n < 0) return SHD_PE_EINVAL;
    std::lock_guard<std::mutex> lk(const_cast<ShdPe*>(pe)->mu);
    for (int32_t k = 0; k < std::min<int32_t>(n, 2); ++k) info[k] = pe->loadInfo[k];
    return SHD_PE_OK;
}

extern "C" int64_t shd_pe_num_arcs(const ShdPe* pe) { return pe ? pe->hg.nArcs() : 0; }

extern "C" int shd_pe_arc_list(const ShdPe* pe, int32_t* from, int32_t* to) {
    if (!pe || !from || !to) return SHD_PE_EINVAL;
    const HostGraph& g = pe->hg;
    for (int32_t u = 0; u < g.n; ++u)
        for (int32_t a = g.rowPtr[(size_t)u]; a < g.rowPtr[(size_t)u + 1]; ++a) {
            from[a] = u;
            to[a] = g.col[(size_t)a];
        }
    return SHD_PE_OK;
}

extern "C" int64_t shd_pe_find_arc(const ShdPe* pe, int32_t from, int32_t to) {
    if (!pe || from < 0 || from >= pe->hg.n || to < 0 || to >= pe->hg.n) return -1;
    return pe->hg.findArc(from, to);
}

extern "C" int shd_pe_paths_info(const ShdPe* pe, int64_t* info, int32_t n) {
    if (!pe || !info || n < 0) return SHD_PE_EINVAL;
    std::lock_guard<std::mutex> lk(const_cast<ShdPe*>(pe)->mu);
    for (int32_t k = 0; k < std::min<int32_t>(n, 7); ++k) info[k] = pe->pathsInfo[k];
    return SHD_PE_OK;
}

extern "C" int shd_pe_paths_set_row_tier(ShdPe* pe, int32_t enable) {
    if (!pe) return SHD_PE_EINVAL;
    std::lock_guard<std::mutex> lk(pe->mu);
    pe->pathsRowTier = enable != 0;
    return SHD_PE_OK;
}

extern "C" int32_t shd_pe_num_shards(const ShdPe* pe) { return pe ? pe->G : 0; }

extern "C" int shd_pe_shard_bounds(const ShdPe* pe, int32_t* bounds) {
    if (!pe || !bounds) return SHD_PE_EINVAL;
    std::memcpy(bounds, pe->bounds.data(), pe->bounds.size() * sizeof(int32_t));
    return SHD_PE_OK;
}

extern "C" int shd_pe_owned_range(const ShdPe* pe, int32_t* start, int32_t* count) {
    if (!pe) return SHD_PE_EINVAL;
    if (start) *start = pe->ownStart;
    if (count) *count = pe->ownEnd - pe->ownStart;
    return SHD_PE_OK;
}

// Streaming copy for the achievable-HBM reference: 16-B
// loads and stores (float4-shaped), each thread moving UNR consecutive-stride
// elements per iteration so UNR loads are in flight before the first store,
// grid-stride over a footprint far past the 256 MiB Infinity Cache.  The
// reference is the best of a few shapes (cache policy x workgroups per CU):
// the figure is what this box's HBM delivers to a well-formed copy.
typedef unsigned int v4u __attribute__((ext_vector_type(4)));
template <bool NT, int UNR>
__global__ __launch_bounds__(256) void k_stream_copy(const v4u* __restrict__ a,
                                                      v4u* __restrict__ b, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i + (UNR - 1) * stride < n; i += UNR * stride) {
        v4u x[UNR];
#pragma unroll
        for (int k = 0; k < UNR; ++k) x[k] = NT ? __builtin_nontemporal_load(&a[i + k * stride]) : a[i + k * stride];
#pragma unroll
        for (int k = 0; k < UNR; ++k) {
            if (NT) __builtin_nontemporal_store(x[k], &b[i + k * stride]);
            else b[i + k * stride] = x[k];
        }
    }
    for (; i < n; i += stride) b[i] = a[i];
}

// one-pass shape: no grid-stride loop, one workgroup per 256 x UNR
// elements (a grid of ~10^5 workgroups), UNR coalesced 4-KiB wave spans per
// thread in flight before the stores
template <bool NT, int UNR>
__global__ __launch_bounds__(256) void k_stream_copy1(const v4u* __restrict__ a,
                                                       v4u* __restrict__ b, size_t n) {
    const size_t base = (size_t)blockIdx.x * 256 * UNR + threadIdx.x;
    v4u x[UNR];
#pragma unroll
    for (int k = 0; k < UNR; ++k) {
        const size_t i = base + (size_t)k * 256;
        if (i < n) x[k] = NT ? __builtin_nontemporal_load(&a[i]) : a[i];
    }
#pragma unroll
    for (int k = 0; k < UNR; ++k) {
        const size_t i = base + (size_t)k * 256;
        if (i < n) {
            if (NT) __builtin_nontemporal_store(x[k], &b[i]);
            else b[i] = x[k];
        }
    }
}

extern "C" int shd_pe_stream_bandwidth(ShdPe* pe, int64_t bytes, int32_t iters, double* gbps) {
    if (!pe || !gbps || bytes < (1 << 20) || iters < 1) return SHD_PE_EINVAL;
    Shard* sh = pe->shards[0].get();
    HIPCHK(hipSetDevice(sh->device));
    const size_t n = (size_t)bytes / 16;
    void *a = nullptr, *b = nullptr;
    if (hipMalloc(&a, n * 16) != hipSuccess) return SHD_PE_ENOMEM;
    if (hipMalloc(&b, n * 16) != hipSuccess) { (void)hipFree(a); return SHD_PE_ENOMEM; }
    int rc = SHD_PE_OK;
    double best = 0.0;
    if (hipMemsetAsync(a, 0, n * 16, sh->stream) != hipSuccess) rc = SHD_PE_EHIP;
    // shapes: cache policy (plain / non-temporal) x 4 or 8 loads in flight per
    // thread x workgroups per CU (SHDPE_STREAM_WG_PER_CU adds one more)
    // plus the one-pass shape (shapes 12..19: policy x 4 / 8 / 2 / 1 per
    // thread; nt with 4 per thread is the best on the boxes seen, ~6.1 TB/s)
    const int wgs[3] = {4, 8, pe->tu.streamWgPerCU};
    for (int shape = 0; shape < 20 && !rc; ++shape) {
        const bool nt = shape & 1;
        const bool onePass = shape >= 12;
        const int unr = shape >= 18 ? 1 : shape >= 16 ? 2 : (shape >> 1) & 1 ? 8 : 4;
        const int grid = onePass ? (int)((n + 256 * (size_t)unr - 1) / (256 * (size_t)unr))
                                 : sh->numCUs * wgs[shape >> 2];
        auto launch = [&]() {
            const v4u* pa = (const v4u*)a;
            v4u* pb = (v4u*)b;
            if (onePass) {
                if (unr == 2 && nt) hipLaunchKernelGGL((k_stream_copy1<true, 2>), dim3(grid), dim3(256), 0, sh->stream, pa, pb, n);
                else if (unr == 2) hipLaunchKernelGGL((k_stream_copy1<false, 2>), dim3(grid), dim3(256), 0, sh->stream, pa, pb, n);
                else if (unr == 1 && nt) hipLaunchKernelGGL((k_stream_copy1<true, 1>), dim3(grid), dim3(256), 0, sh->stream, pa, pb, n);
                else if (unr == 1) hipLaunchKernelGGL((k_stream_copy1<false, 1>), dim3(grid), dim3(256), 0, sh->stream, pa, pb, n);
                else if (nt && unr == 8) hipLaunchKernelGGL((k_stream_copy1<true, 8>), dim3(grid), dim3(256), 0, sh->stream, pa, pb, n);
                else if (nt) hipLaunchKernelGGL((k_stream_copy1<true, 4>), dim3(grid), dim3(256), 0, sh->stream, pa, pb, n);
                else if (unr == 8) hipLaunchKernelGGL((k_stream_copy1<false, 8>), dim3(grid), dim3(256), 0, sh->stream, pa, pb, n);
                else hipLaunchKernelGGL((k_stream_copy1<false, 4>), dim3(grid), dim3(256), 0, sh->stream, pa, pb, n);
            } else if (nt && unr == 8) hipLaunchKernelGGL((k_stream_copy<true, 8>), dim3(grid), dim3(256), 0, sh->stream, pa, pb, n);
            else if (nt) hipLaunchKernelGGL((k_stream_copy<true, 4>), dim3(grid), dim3(256), 0, sh->stream, pa, pb, n);
            else if (unr == 8) hipLaunchKernelGGL((k_stream_copy<false, 8>), dim3(grid), dim3(256), 0, sh->stream, pa, pb, n);
            else hipLaunchKernelGGL((k_stream_copy<false, 4>), dim3(grid), dim3(256), 0, sh->stream, pa, pb, n);
        };
        launch();   // warm-up
        (void)hipEventRecord(sh->evA, sh->stream);
        for (int i = 0; i < iters; ++i) launch();
        (void)hipEventRecord(sh->evB, sh->stream);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(sh->stream) != hipSuccess) {
            rc = SHD_PE_EHIP;
            break;
        }
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, sh->evA, sh->evB);
        const double gb = ms > 0.f ? 2.0 * (double)n * 16.0 * iters / (ms * 1e-3) / 1e9 : 0.0;
        if (pe->tu.debug)
            std::fprintf(stderr, "[shdpe] stream shape %d (%s, %d per thread, grid %d): %.0f GB/s\n", shape,
                         nt ? "nt" : "plain", unr, grid, gb);
        best = std::max(best, gb);
    }
    if (!rc) *gbps = best;
    (void)hipFree(a);
    (void)hipFree(b);
    return rc;
}

extern "C" int shd_pe_synchronize(ShdPe* pe) {
    if (!pe) return SHD_PE_EINVAL;
    for (auto& s : pe->shards) {
        HIPCHK(hipSetDevice(s->device));
        HIPCHK(hipStreamSynchronize(s->stream));
    }
    return SHD_PE_OK;
}

extern "C" void shd_pe_destroy(ShdPe* pe) {
    if (!pe) return;
    for (auto& s : pe->shards) destroy_shard(s.get());
    if (pe->xcomm) (void)ncclCommDestroy(pe->xcomm);
    for (unsigned char* h : pe->stage)
        if (h) (void)hipHostFree(h);
    delete pe;
}

extern "C" int shd_pe_is_complete(const ShdPe* pe) { return pe && pe->hg.isComplete ? 1 : 0; }

extern "C" int32_t shd_pe_num_attached(const ShdPe* pe) {
    return pe ? (int32_t)pe->attached.size() : 0;
}

extern "C" int shd_pe_attached(const ShdPe* pe, int32_t* out) {
    if (!pe || !out) return SHD_PE_EINVAL;
    std::memcpy(out, pe->attached.data(), pe->attached.size() * sizeof(int32_t));
    return SHD_PE_OK;
}

extern "C" int shd_pe_get_stats(const ShdPe* pe, ShdPeStats* out) {
    if (!pe || !out) return SHD_PE_EINVAL;
    // compute updates the per-shard stats under mu: snapshot under it too
    // (a call during a compute returns once that compute is done)
    std::lock_guard<std::mutex> lk(const_cast<ShdPe*>(pe)->mu);
    ShdPeStats t = pe->shards[0]->stats;
    for (size_t i = 1; i < pe->shards.size(); ++i) {
        const ShdPeStats& s = pe->shards[i]->stats;
        t.rowsComputed += s.rowsComputed;
        t.rowsExact += s.rowsExact;
        t.rowsTieEarly += s.rowsTieEarly;
        t.rowsTieRepaired += s.rowsTieRepaired;
        t.arcsRelaxed += s.arcsRelaxed;
        t.msSparseKernel += s.msSparseKernel;
        t.msExactKernel += s.msExactKernel;
        t.msDirectKernel += s.msDirectKernel;
        t.msTotal = std::max(t.msTotal, s.msTotal);   // shards run concurrently
        t.launchesSparse += s.launchesSparse;
        t.launchesExact += s.launchesExact;
        t.launchesDirect += s.launchesDirect;
        t.msDenseKernel += s.msDenseKernel;
        t.launchesDense += s.launchesDense;
        t.denseSweeps += s.denseSweeps;
        t.denseFlops += s.denseFlops;
    }
    t.nShards = (int32_t)pe->shards.size();
    t.msGather = pe->msGather;
    *out = t;
    return SHD_PE_OK;
}

extern "C" int64_t shd_pe_stats_size(void) { return (int64_t)sizeof(ShdPeStats); }

extern "C" int shd_pe_get_stats_sized(const ShdPe* pe, void* out, int64_t outBytes) {
    if (!pe || !out || outBytes <= 0) return SHD_PE_EINVAL;
    ShdPeStats t;
    const int rc = shd_pe_get_stats(pe, &t);
    if (rc) return rc;
    std::memcpy(out, &t, (size_t)std::min<int64_t>(outBytes, (int64_t)sizeof(ShdPeStats)));
    return SHD_PE_OK;
}

extern "C" int shd_pe_reset_stats(ShdPe* pe) {
    if (!pe) return SHD_PE_EINVAL;
    std::lock_guard<std::mutex> lk(pe->mu);
    for (auto& sp : pe->shards) {
        ShdPeStats& st = sp->stats;
        ShdPeStats keep = st;
        std::memset(&st, 0, sizeof(st));
        st.mode = keep.mode;
        st.isComplete = keep.isComplete;
        st.nVertices = keep.nVertices;
        st.nArcs = keep.nArcs;
        st.nAttached = keep.nAttached;
        st.deltaUsed = keep.deltaUsed;
        st.batched = keep.batched;
        st.batchLanes = keep.batchLanes;
        st.batchWaves = keep.batchWaves;
        st.batchPostWaves = keep.batchPostWaves;
        sp->predClaimed = sp->predGathered = 0;
        sp->redoBatches = 0;
        sp->roundsRun = sp->batchesRun = 0;
    }
    pe->msGather = 0.0;
    return SHD_PE_OK;
}

extern "C" int shd_pe_pred_filter_counts(const ShdPe* pe, int64_t* claimed, int64_t* gathered) {
    if (!pe || !claimed || !gathered) return SHD_PE_EINVAL;
    std::lock_guard<std::mutex> lk(const_cast<ShdPe*>(pe)->mu);
    *claimed = *gathered = 0;
    for (auto& sp : pe->shards) {
        *claimed += sp->predClaimed;
        *gathered += sp->predGathered;
    }
    return SHD_PE_OK;
}

extern "C" int shd_pe_post_split_info(const ShdPe* pe, int32_t* split, int32_t* labelWaves,
                                      int64_t* redoBatches) {
    if (!pe || !split || !labelWaves || !redoBatches) return SHD_PE_EINVAL;
    std::lock_guard<std::mutex> lk(const_cast<ShdPe*>(pe)->mu);
    *split = *labelWaves = 0;
    *redoBatches = 0;
    // (before the first compute the plan holds configure's pick; ensure_batch
    // may still drop the split when the label arrays do not fit)
    if (pe->batched && !pe->shards.empty()) {
        const shdpe::Shard& sh = *pe->shards[0];
        *split = sh.plan.relax.split && sh.plan.postSplit && (!sh.batchReady || sh.postSplitOk) ? 1 : 0;
        *labelWaves = *split ? sh.plan.label.wpe : 0;
    }
    for (auto& sp : pe->shards) *redoBatches += sp->redoBatches;
    return SHD_PE_OK;
}

extern "C" int shd_pe_batch_info(const ShdPe* pe, int32_t shard, int64_t out[4]) {
    if (!pe || !out || shard < 0 || (size_t)shard >= pe->shards.size()) return SHD_PE_EINVAL;
    std::lock_guard<std::mutex> lk(const_cast<ShdPe*>(pe)->mu);
    const shdpe::Shard& sh = *pe->shards[(size_t)shard];
    // (batchRound / batchSlots: 0 until ensure_batch ran, at the shard's first batched compute)
    out[0] = sh.batchRound;
    out[1] = sh.batchSlots;
    out[2] = sh.roundsRun;
    out[3] = sh.batchesRun;
    return SHD_PE_OK;
}

extern "C" int shd_pe_sparse_info(const ShdPe* pe, int32_t shard, int64_t out[8]) {
    if (!pe || !out || shard < 0 || (size_t)shard >= pe->shards.size()) return SHD_PE_EINVAL;
    const shdpe::SparseLaunch& c = pe->shards[(size_t)shard]->cfg;    // (written by configure only)
    out[0] = c.layout;
    out[1] = c.threads;
    out[2] = c.qcap;
    out[3] = c.hcap;
    out[4] = c.heavyDeg;
    out[5] = shdpe::sparse_lanes_per_vertex(c);
    out[6] = c.kflags;
    out[7] = c.grid;
    return SHD_PE_OK;
}

extern "C" int shd_pe_direct_path(const ShdPe* pe, int32_t s, int32_t t, double* lat,
                                  double* rel) {
    if (!pe) return SHD_PE_EINVAL;
    return host_direct_path(pe->hg, s, t, lat, rel);
}

extern "C" int shd_pe_self_path(const ShdPe* pe, int32_t v, double* lat, double* rel) {
    if (!pe) return SHD_PE_EINVAL;
    return host_self_path(pe->hg, v, lat, rel);
}

extern "C" int shd_pe_adjacent(const ShdPe* pe, int32_t s, int32_t t) {
    if (!pe) return 0;
    return pe->hg.findArc(s, t) != -1 ? 1 : 0;
}

// ---- batched helpers (pe_aux.hip) ----------------------------------------
// Inputs / outputs are host arrays; chunks of up to 16M entries are staged
// through device buffers owned by the call, on shard 0's device and stream.
namespace {
struct AuxBufs {
    void* p[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    ~AuxBufs() { for (void* x : p) if (x) (void)hipFree(x); }
};
constexpr int64_t AUX_CHUNK = (int64_t)1 << 24;
}  // namespace

extern "C" int shd_pe_self_paths(ShdPe* pe, const int32_t* vertices, int32_t count, double* lat,
                                 double* rel, uint8_t* flags) {
    if (!pe || count < 0 || (count > 0 && (!vertices || !lat || !rel || !flags))) return SHD_PE_EINVAL;
    if (count == 0) return SHD_PE_OK;
    std::lock_guard<std::mutex> lk(pe->mu);
    Shard* sh = pe->shards[0].get();
    HIPCHK(hipSetDevice(sh->device));
    const int64_t ch = std::min<int64_t>(count, AUX_CHUNK);
    AuxBufs b;
    if (hipMalloc(&b.p[0], ch * 4) || hipMalloc(&b.p[1], ch * 8) || hipMalloc(&b.p[2], ch * 8) ||
        hipMalloc(&b.p[3], ch))
        return SHD_PE_ENOMEM;
    for (int64_t c0 = 0; c0 < count; c0 += ch) {
        const int32_t c = (int32_t)std::min<int64_t>(ch, count - c0);
        HIPCHK(hipMemcpyAsync(b.p[0], vertices + c0, (size_t)c * 4, hipMemcpyHostToDevice, sh->stream));
        launch_self_paths(sh->dgAux, (const int32_t*)b.p[0], c, pe->hg.nEdges, (double*)b.p[1],
                          (double*)b.p[2], (uint8_t*)b.p[3], sh->stream);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(lat + c0, b.p[1], (size_t)c * 8, hipMemcpyDeviceToHost, sh->stream));
        HIPCHK(hipMemcpyAsync(rel + c0, b.p[2], (size_t)c * 8, hipMemcpyDeviceToHost, sh->stream));
        HIPCHK(hipMemcpyAsync(flags + c0, b.p[3], (size_t)c, hipMemcpyDeviceToHost, sh->stream));
        HIPCHK(hipStreamSynchronize(sh->stream));
    }
    return SHD_PE_OK;
}

static int pairs_call(ShdPe* pe, const int32_t* src, const int32_t* dst, int64_t count, int mode,
                      double* lat, double* rel, uint8_t* flags) {
    if (!pe || count < 0 || (count > 0 && (!src || !dst || !flags || (mode == 0 && (!lat || !rel)))))
        return SHD_PE_EINVAL;
    if (count == 0) return SHD_PE_OK;
    std::lock_guard<std::mutex> lk(pe->mu);
    Shard* sh = pe->shards[0].get();
    HIPCHK(hipSetDevice(sh->device));
    const int64_t ch = std::min<int64_t>(count, AUX_CHUNK);
    AuxBufs b;
    if (hipMalloc(&b.p[0], ch * 4) || hipMalloc(&b.p[1], ch * 4) || hipMalloc(&b.p[4], ch) ||
        (mode == 0 && (hipMalloc(&b.p[2], ch * 8) || hipMalloc(&b.p[3], ch * 8))))
        return SHD_PE_ENOMEM;
    for (int64_t c0 = 0; c0 < count; c0 += ch) {
        const int64_t c = std::min<int64_t>(ch, count - c0);
        HIPCHK(hipMemcpyAsync(b.p[0], src + c0, (size_t)c * 4, hipMemcpyHostToDevice, sh->stream));
        HIPCHK(hipMemcpyAsync(b.p[1], dst + c0, (size_t)c * 4, hipMemcpyHostToDevice, sh->stream));
        launch_pairs(sh->dgAux, (const int32_t*)b.p[0], (const int32_t*)b.p[1], c, mode,
                     (double*)b.p[2], (double*)b.p[3], (uint8_t*)b.p[4], sh->stream);
        HIPCHK(hipGetLastError());
        if (mode == 0) {
            HIPCHK(hipMemcpyAsync(lat + c0, b.p[2], (size_t)c * 8, hipMemcpyDeviceToHost, sh->stream));
            HIPCHK(hipMemcpyAsync(rel + c0, b.p[3], (size_t)c * 8, hipMemcpyDeviceToHost, sh->stream));
        }
        HIPCHK(hipMemcpyAsync(flags + c0, b.p[4], (size_t)c, hipMemcpyDeviceToHost, sh->stream));
        HIPCHK(hipStreamSynchronize(sh->stream));
    }
    return SHD_PE_OK;
}

extern "C" int shd_pe_direct_paths(ShdPe* pe, const int32_t* src, const int32_t* dst, int64_t count,
                                   double* lat, double* rel, uint8_t* flags) {
    return pairs_call(pe, src, dst, count, 0, lat, rel, flags);
}

extern "C" int shd_pe_adjacent_pairs(ShdPe* pe, const int32_t* src, const int32_t* dst,
                                     int64_t count, uint8_t* out) {
    return pairs_call(pe, src, dst, count, 1, nullptr, nullptr, out);
}

extern "C" int shd_pe_is_complete_device(ShdPe* pe, int32_t* isComplete) {
    if (!pe || !isComplete) return SHD_PE_EINVAL;
    std::lock_guard<std::mutex> lk(pe->mu);
    Shard* sh = pe->shards[0].get();
    HIPCHK(hipSetDevice(sh->device));
    AuxBufs b;
    if (hipMalloc(&b.p[0], 4)) return SHD_PE_ENOMEM;
    const int32_t init = INT32_MAX;
    HIPCHK(hipMemcpyAsync(b.p[0], &init, 4, hipMemcpyHostToDevice, sh->stream));
    const std::vector<int32_t>& ec = pe->hg.edgeCount;    // multigraphs: edge counts
    if (!ec.empty()) {
        if (hipMalloc(&b.p[1], ec.size() * 4)) return SHD_PE_ENOMEM;
        HIPCHK(hipMemcpyAsync(b.p[1], ec.data(), ec.size() * 4, hipMemcpyHostToDevice, sh->stream));
    }
    launch_incident_min(sh->dgAux, ec.empty() ? nullptr : (const int32_t*)b.p[1], (int32_t*)b.p[0], sh->stream);
    HIPCHK(hipGetLastError());
    int32_t mn = 0;
    HIPCHK(hipMemcpyAsync(&mn, b.p[0], 4, hipMemcpyDeviceToHost, sh->stream));
    HIPCHK(hipStreamSynchronize(sh->stream));
    *isComplete = mn >= pe->hg.n ? 1 : 0;
    return SHD_PE_OK;
}

// exported for the host topology mirror (pe_topology.cpp)
const shdpe::HostGraph* shd_pe_host_graph(const ShdPe* pe) { return pe ? &pe->hg : nullptr; }
int32_t shd_pe_position(const ShdPe* pe, int32_t v) {
    return (pe && v >= 0 && v < pe->hg.n) ? pe->posOf[v] : -1;
}
