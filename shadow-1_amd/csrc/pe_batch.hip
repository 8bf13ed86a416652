// pe_batch.hip -- batched multi-source sparse kernel of the Shadow path
// engine (gfx950).
//
// Reference semantics (Shadow v1.14.0, src/main/routing/topology.c): one
// source row = _topology_computeSourcePaths (:1655-1875) = igraph 0.7.1
// Dijkstra (:1765) + the per-target fold _topology_computePathProperties
// (:1407-1523).  Same contract as k_sparse_rows (pe_kernels.hip); this kernel
// is the layout for graphs whose per-row state does not fit LDS (n of 10^5+).
//
// One workgroup owns a batch of LB sources.  Every per-vertex array is laid
// out [v][LB]: a group of LB lanes handles one vertex for all LB sources
// (lane l = source l), so one arc relaxation dist[u] + w -> dist[v] for LB
// sources is ONE coalesced LB*8-byte access instead of LB random ones.  The
// per-source distance rows (0.8-2 MB each) live in HBM; loaded latency is
// ~1.2 us per dependent access, so every stage keeps several independent
// vertices per group in flight (V-way interleave) and the relaxation phase
// carries no labels at all.  Sources of a batch are chosen close together in
// the graph (host-side BFS rank), so their bucket frontiers coincide.
//
// Per batch:
//   1. label-correcting delta-stepping over per-lane keys (dist + the lane's
//      shift: sources of one batch share a nearest hub, and the shift aligns
//      their distances behind it) with one bucket bound, a near and a far
//      pending bitmap (one bit per vertex), and per-ENTRY dirty bits: an entry
//      is relaxed once per value it takes (dirty -> clean by CAS), not once per
//      visit of its vertex; relaxations are dist[u] + w only (left fold ->
//      igraph's distances bit for bit);
//   2. predecessor pass: tight in-arc with minimum dist[u] per lane = igraph's
//      first-popped tight predecessor; equal minima (or a zero-increment arc)
//      mark the entry ambiguous (the row becomes a tie row for k_exact_rows
//      if a target's path meets it);
//   3. labels on demand + the row writer (topology.c:1805-1864): each lane
//      walks its targets' predecessor chains up to the first entry with
//      known labels and unwinds them (hops + 1, rel * r: the reference's left
//      fold, topology.c:1430, :1499, exactly), keeping every label it
//      derives -- only the ~27% of entries on target paths (C4) are touched;
//   4. tie export for rows whose target paths meet an ambiguous entry.
#include <hip/hip_runtime.h>

#include "pe_bucket.hpp"
#include "pe_device.hpp"
#include "pe_devutil.hpp"

namespace shdpe {

constexpr int BT_THREADS = 1024;
constexpr int BK = 3;        // arcs per vertex per load batch (relaxation)
constexpr int BKP = 3;       // in-arcs per vertex per load batch (predecessor pass)
constexpr int PRED_HEAVY = 64;   // predecessor pass: in-degree of a wave-scanned entry
// WPE = waves per SIMD the kernel is compiled for: 4 (128 VGPRs, one
// 1024-thread workgroup per CU, two vertices interleaved per group) or 8
// (64 VGPRs, two workgroups per CU, one vertex per group)
// (experiment knobs for same-box A/B builds, tools/build_variant.sh -D...)
#ifndef SHDPE_W4_BV
#define SHDPE_W4_BV 2
#endif
#ifndef SHDPE_W4_BK
#define SHDPE_W4_BK 3
#endif
template <int WPE> struct BCfg {
    static constexpr int BV = WPE >= 6 ? 1 : SHDPE_W4_BV;   // vertices interleaved per group
    static constexpr int SMAX = WPE >= 6 ? 8 : 16;   // label-walk stack: (entry, arc) pairs per thread
    static constexpr int BKR = WPE >= 6 ? BK : SHDPE_W4_BK;   // dist gathers per vertex in flight
    static constexpr int BKQ = WPE >= 6 ? BKP : SHDPE_W4_BK;
};
constexpr int WALK_BUDGET = 2048;   // walk steps per target before the deep-tree sweeps
// Lane policy of the relaxation: a vertex with ANY dirty lane below the
// bucket bound relaxes ALL its dirty lanes (eager) instead of only those
// below the bound.  The lanes of a batch reach a vertex in different
// buckets; taking the late ones along with the first costs some label-
// correcting re-relaxations but saves whole vertex visits (each visit reads
// one [v][LB] line per arc): C4 schedule simulation (tools/sim) 2.21 -> 1.56
// arc visits per batch, x m_arcs, at a quarter of the bucket width.
constexpr bool EAGER = true;

struct alignas(16) BCtrl {
    int qtail;
    int farAny;       // some vertex waits in the far set
    unsigned long long farMin;   // smallest far key (bits of a non-negative double)
    unsigned int ambMask;
    int changed;
    int htail;        // heavy-vertex list (grows down from the top of the queue)
    int qhead;        // next light-queue entry to take (dynamic distribution)
    unsigned long long busyMax;
    unsigned long long busySum;
    double maxOff;    // largest lane offset of the batch (bits via atomicMax)
    // SHD_PE_DEBUG_COUNTERS only: vertex processings, arcs, active lanes and
    // the relax / predecessor phase timestamps (in LDS, not registers: the
    // relax loop runs at its VGPR cap)
    unsigned int dProcs, dArcs, dLanes;
    unsigned int dWhy;   // SHDPE_DIAG_WHY builds: why the batch's rows left the fast path
    long long t0, t1, t2, t3, t4;
    // SHD_PE_DEBUG_COUNTERS only: in-arcs of the entries the on-demand
    // predecessor pass claimed, and the in-arcs it gathered (the filter)
    unsigned int dClaim, dGath;
};
static_assert(sizeof(BCtrl) <= 128, "batch control block");
constexpr int BCTRL_BYTES = 128;

// PART 5 (predecessor part): entries of its heavy list, behind the pending
// bitmaps in an LDS of its own size (batch_lds_bytes): 4,096, fewer when the
// bitmaps leave less of the CU's 160 KB (1 KB of which stays free for the
// kernel's static __shared__ arrays -- tieSlot, laneRow, tieThr, nextB, 516 B
// at LB 32: a dynamic size that fills the whole LDS makes the launch invalid)
__host__ __device__ constexpr int pred_heavy_cap(int nwp, bool gbits) {
    const int room = (160 * 1024 - 1024 - BCTRL_BYTES - (gbits ? 0 : 8 * nwp)) / 4;
    return room < 0 ? 0 : room < 4096 ? room : 4096;
}

// SHDPE_DIAG_WHY (diagnostic builds only, tools/build_variant.sh -D...): per
// batch, the reasons its rows went to the exact kernel, in dbg[16 b + 1]:
// 1 failed, 2 Bellman violation in the on-demand predecessor pass, 4 in the
// full pass, 8 a label walk met an entry without a parent (or the never-spin
// cap), 16 a walk met an ambiguous entry, 32 deep tree (sweeps), 64 the full
// pass ran (attempt 1), 128 the relax kernel flagged the batch (phase cap)
#ifdef SHDPE_DIAG_WHY
#define DIAG_WHY(bit) (why |= (bit))
// the first phase-2 violations of the first batches: entry, stored distance,
// the in-arc minimum that undercuts it (printf; diagnostic builds only)
#define DIAG_VIOL(b, v, lane, dv, mnv, hv)                                                     \
    do {                                                                                    \
        if ((b) < 6 && atomicAdd(&sDiagViol, 1) < 4)                                        \
            printf("[diag] viol batch %d v %d lane %d dist %.17g min %.17g heavy %d attempt %d\n", \
                   (b), (v), (lane), b2d(dv), b2d(mnv), (hv), attempt);                     \
    } while (0)
#else
#define DIAG_WHY(bit) ((void)0)
#define DIAG_VIOL(b, v, lane, dv, mnv, hv) ((void)0)
#endif

// Entry encoding of the [v][LB] distance array: (f64 bits << 1) | dirty.
// Positive doubles have bit 63 clear, so the shift loses nothing and the u64
// order of encodings is the order of distances: an atomic min with a dirty
// encoding of a smaller distance always wins, an equal or larger one never
// changes the entry (an equal distance does not re-dirty a clean entry:
// clean = bit 0 clear is the smaller encoding).  A processor marks the value
// it relaxed clean with a no-return atomic min of e & ~1: if an improvement
// landed in between, its encoding is below e & ~1 and stays, dirty.
__device__ __forceinline__ unsigned long long enc_dirty(unsigned long long bits) { return (bits << 1) | 1ull; }
__device__ __forceinline__ unsigned long long dec(unsigned long long e) { return e >> 1; }
__device__ __forceinline__ bool is_dirty(unsigned long long e) { return (e & 1ull) != 0; }
constexpr unsigned long long INF_ENC = INF_BITS << 1;   // +inf, clean

// (perturbation variants of these three -- plain stores, doubled atomics,
// doubled reads -- are patches under tools/variants/, built by
// tools/build_variant.sh for same-box A/B runs)
__device__ __forceinline__ unsigned long long ld_d(unsigned long long* p) { return ld_wg(p); }

__device__ __forceinline__ void relax_min(unsigned long long* p, unsigned long long v) {
    __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// relax pre-check load
__device__ __forceinline__ unsigned long long relax_ld(unsigned long long* D, int x, int LB, int l) {
    return ld_d(&D[(size_t)x * LB + l]);
}

__device__ __forceinline__ void mark_clean(unsigned long long* p, unsigned long long e) {
    __hip_atomic_fetch_min(p, e & ~1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// Pending bitmaps (one bit per vertex, near + far sets): in LDS when both
// fit beside the control block (n <= ~655k), else in the slot's global
// scratch (GB): same operations at workgroup scope.
template <bool GB> struct Bits;
template <> struct Bits<false> {
    uint32_t* p;
    __device__ __forceinline__ uint32_t ld(int w) const { return p[w]; }
    __device__ __forceinline__ void st(int w, uint32_t v) const { p[w] = v; }
    __device__ __forceinline__ void set(int v) const { atomicOr(&p[v >> 5], 1u << (v & 31)); }
    // sets the bit, returns whether it was set before
    __device__ __forceinline__ bool test_set(int v) const {
        return (atomicOr(&p[v >> 5], 1u << (v & 31)) >> (v & 31)) & 1u;
    }
};
template <> struct Bits<true> {
    uint32_t* p;
    __device__ __forceinline__ uint32_t ld(int w) const { return ld_wg(&p[w]); }
    __device__ __forceinline__ void st(int w, uint32_t v) const {
        __hip_atomic_store(&p[w], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __device__ __forceinline__ void set(int v) const {
        __hip_atomic_fetch_or(&p[v >> 5], 1u << (v & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __device__ __forceinline__ bool test_set(int v) const {
        return (__hip_atomic_fetch_or(&p[v >> 5], 1u << (v & 31), __ATOMIC_RELAXED,
                                      __HIP_MEMORY_SCOPE_WORKGROUP) >> (v & 31)) & 1u;
    }
};

// Wave-aggregated append of `val` (lanes with `want`) to a list whose tail
// counter lives in LDS: one LDS atomic per wave.
__device__ __forceinline__ void wave_append(int32_t* Q, int* tail, bool want, int val) {
    const uint64_t m = __ballot(want);
    if (!m) return;
    const int lane = (int)(threadIdx.x & 63);
    const int leader = __ffsll((unsigned long long)m) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(tail, __popcll(m));
    base = __shfl(base, leader, 64);
    if (want) __hip_atomic_store(&Q[base + __popcll(m & ((1ull << lane) - 1))], val, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_WORKGROUP);
}

// workgroup-uniform values read from LDS, pinned to scalar registers (the
// relax loop runs at its VGPR cap)
__device__ __forceinline__ int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ double uni(double x) {
    const long long b = __double_as_longlong(x);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)b);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(b >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

__device__ __forceinline__ void st_wg(int32_t* p, int v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void st_wg(double* p, double v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void st_wg(unsigned long long* p, unsigned long long v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// label records (BLabel): two 8-B halves of one 16-B slot, loaded / stored
// with relaxed workgroup-scope accesses (walks of other groups race on them:
// a half-written record reads as unresolved -- hop label -1 or rel < 0 --
// and the reader walks on, as the labels are written once with the only
// value the fold can give)
struct Lbl {
    double rel;
    int hops, arc;
};
__device__ __forceinline__ Lbl lbl_ld(BLabel* p) {
    const unsigned long long x = ld_wg(&p->ha);
    return Lbl{ld_wg(&p->rel), (int)(unsigned)x, (int)(unsigned)(x >> 32)};
}
__device__ __forceinline__ int lbl_arc(BLabel* p) { return (int)(unsigned)(ld_wg(&p->ha) >> 32); }
__device__ __forceinline__ void lbl_st(BLabel* p, double rel, int hops, int arc) {
    st_wg(&p->rel, rel);
    st_wg(&p->ha, (unsigned long long)(unsigned)hops | ((unsigned long long)(unsigned)arc << 32));
}
__device__ __forceinline__ bool lbl_known(const Lbl& x) { return x.hops >= 0 && x.rel >= 0.0; }

// Forward reliability fold with vertex factors (topology.c:1430-1462, :1499)
// along lane l's predecessor chain, multiplied in source -> target order:
// the chain is walked in blocks of 64 factors from the source end (O(h)
// loads per block, O(h^2 / 64) in all; no per-thread scratch beyond 64).
template <int LB>
__device__ __noinline__ double fold_rel_batch(const double* __restrict__ vrel,
                                              const double* __restrict__ inRel,
                                              const int32_t* __restrict__ inCol,
                                              BLabel* LBL, int l, int s, int t, int h) {
    // (arrays by value: a DevGraph& would pin the caller's descriptor in scratch)
    double acc = 1.0 * vrel[s];
    acc = acc * vrel[t];
    for (int lo = 0; lo < h; lo += 64) {        // hops (lo, hi] counted from the source
        const int hi = min(h, lo + 64);
        int x = t;
        for (int up = 0; up < h - hi; ++up) x = inCol[lbl_arc(&LBL[(size_t)x * LB + l]) & ~TIE_AMB];
        double fac[64];
        int k = 0;
        while (k < hi - lo) {
            const int a = lbl_arc(&LBL[(size_t)x * LB + l]) & ~TIE_AMB;
            fac[k++] = inRel[a];
            x = inCol[a];
        }
        for (int i = k - 1; i >= 0; --i) acc = acc * fac[i];
    }
    return acc;
}

// k_batch_rows<LB, WPE, GB, PART>.  PART 0 is the whole batch in one kernel; the
// others split it over a round of batches whose dist arrays persist in HBM (slot
// = batch index), each with its own register budget and LDS, ordered by the
// stream; only the batch's flag word crosses.  PART 5 / 6 keep label records
// per BATCH (bs.LB).  ON DEMAND = only vertices on some target's path.
//   PART  init             relax  predecessors            labels, rows            ties          then
//   0     fill, seed       yes    full; repair -> relax   walks, sweeps, rows     in line
//   1     fill, seed       yes    -                       -                       -             flush_hits, flags
//   2     failed <- flags  -      on demand, then full    walks | sweeps, rows    request|line
//   4     as 2 (shd_pe_get_paths' pass: distances, ambiguity bytes, tie export; no row stores)
//   5     failed <- flags  -      on demand               -                       -             failed -> flags
//   6     failed <- flags  -      -                       walks, rows | redo      request
// PART 2's second attempt (full pass) serves a tree deeper than WALK_BUDGET or a
// tie batch without a deferred-export buffer; PART 6 writes no row for such a
// batch and appends it to bs.redo; PART 2 with bs.redoRun runs over that list.
template <int PART> struct PartTraits {
    static constexpr bool relax_part = PART == 1, pred_part = PART == 5, label_part = PART == 6;
    static constexpr bool relaxes = PART == 0 || PART == 1;
    static constexpr bool round_arrays = PART != 0;        // dist arrays per batch of the round
    static constexpr bool has_labels_in_bs = pred_part || label_part;   // label records per batch too (bs.LB)
    static constexpr bool uses_bitmaps = !label_part;
    static constexpr bool reads_relax_flags = PART >= 2;   // bs.flags[b]: failed, in-arc flags written
    static constexpr bool runs_pred_pass = !relax_part && !label_part;
    static constexpr bool writes_rows = PART != 4;
    static constexpr bool defers_ties = PART >= 2;         // k_tie_export after the kernel, if it has a buffer
    static constexpr bool exports_ties = !relax_part && !pred_part;
};

// candidates = vertices with a near bit (consumed)
// (hubs -- degree >= the engine's heavy threshold -- go to a list
// of their own, processed by whole waves: one 16-lane group on a
// hub's ~1000 arcs would set the phase's length)
template <int NT, bool GB>
__device__ __forceinline__ void list_near(const Bits<GB> anyC, const uint32_t* heavyBits, BCtrl* ctl, int32_t* Q, size_t NS,
                                          int nw, int tid) {
    for (int w = tid; w < nw; w += NT) {
        uint32_t bits = anyC.ld(w);
        if (bits) {
            anyC.st(w, 0u);
            uint32_t hv = bits & heavyBits[w];
            bits &= ~hv;
            if (bits) {
                int pos = atomicAdd(&ctl->qtail, __popc(bits));
                while (bits) {
                    const int bb = __ffs(bits) - 1;
                    bits &= bits - 1;
                    Q[pos++] = (w << 5) + bb;
                }
            }
            if (hv) {
                int pos = atomicAdd(&ctl->htail, __popc(hv));
                while (hv) {
                    const int bb = __ffs(hv) - 1;
                    hv &= hv - 1;
                    Q[NS - 1 - pos++] = (w << 5) + bb;
                }
            }
        }
    }
}

// the batch's in-arc flags, LDS -> HBM (bit 1 of the flag word: written)
template <int NT>
__device__ __forceinline__ void flush_hits(const uint32_t* hb, uint32_t* AHw, int64_t mStride, int tid) {
    fence_wg();
    __syncthreads();
    const uint4* const H4 = reinterpret_cast<const uint4*>(hb);
    uint4* const G4 = reinterpret_cast<uint4*>(AHw);
    const int cnt16 = (int)(mStride >> 7);
    for (int i = tid; i < cnt16; i += NT) G4[i] = H4[i];
}

template <int LB, int WPE, bool GB, int PART>
__global__ __launch_bounds__(BT_THREADS) __attribute__((amdgpu_waves_per_eu(WPE)))
void k_batch_rows(DevGraph g0, DevTable tab0, BatchScratch bs, const int32_t* __restrict__ batchRows, int32_t nBatches,
                  uint8_t* rowAmbig, double delta, int32_t* dbg, const TieBuf* __restrict__ tieDesc) {
    using P = PartTraits<PART>;
    // the plain relax with LDS bitmaps flags in-arcs for the predecessor filter
    constexpr bool HITS = PART == 1 && !GB;
    constexpr int BV = BCfg<WPE>::BV, SMAX = BCfg<WPE>::SMAX;
    // the light-vertex relax loop and the predecessor pass are software-
    // pipelined three takes deep with lane-distributed arc records (round 5:
    // C4 N=1 106 -> 98.4 ms, N=8 shards 19.4 -> 18.9 ms same box, r05f;
    // profiles/r05_ab_notes.txt); BKR / BKQ = dist gathers per vertex in flight
    constexpr int BKR = BCfg<WPE>::BKR, BKQ = BCfg<WPE>::BKQ;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int tieSlot[LB];
    __shared__ int laneRow[LB];           // table row of each lane (-1: pad)
    __shared__ unsigned long long tieThr[LB];
    const DevGraph g = global_view(g0);
    const DevTable tab = global_view(tab0);
    constexpr unsigned int LBMASK = LB >= 32 ? 0xFFFFFFFFu : ((1u << (LB & 31)) - 1u);
    const int n = g.n;
    const int nw = (n + 31) >> 5;
    const int nwp = (nw + 3) & ~3;
    // the workgroup size is part of the variant (batch_threads, which
    // launch_batch_rows launches with): a compile-time NT makes every stride, group count and LDS tile offset a
    // constant instead of a live register (round 6: fewer spills in the
    // post kernels' loops)
    constexpr int NT = WPE == 6 ? 768 : BT_THREADS;
    const int tid = threadIdx.x;
    const int l = tid % LB;
    const int gid = tid / LB, NG = NT / LB;
    const int gbase = (tid & 63) - l;       // first lane of my group in the wave
    const bool undirected = g.inCol == g.col;
    const size_t NE = (size_t)n * LB;        // (vertex, lane) entries

    BCtrl* ctl = reinterpret_cast<BCtrl*>(smem);
    uint32_t* const bits0 = GB ? as_global(bs.bits) + (size_t)blockIdx.x * 2 * nwp
                               : reinterpret_cast<uint32_t*>(smem + BCTRL_BYTES);
    const Bits<GB> any0{bits0}, any1{bits0 + nwp};

    const size_t slot = blockIdx.x;
    const size_t NS = (size_t)bs.nStride;
    const size_t SE = NS * LB;
    unsigned long long* D = as_global(bs.D + slot * SE);
    BLabel* LBL = as_global(bs.L + slot * SE);
    int32_t* Q = as_global(bs.queue + slot * NS);

    // batches are taken from a device counter (dynamic: a batch's cost varies
    // by ~20%, and a workgroup finishing early takes the next one)
    __shared__ int nextB;
    for (;;) {
        if (tid == 0) nextB = atomicAdd(bs.next, 1);
        __syncthreads();
        int b = nextB;
        if (PART == 2 && bs.redoRun) {     // the redo launch: the batches PART 6 listed
            if (b >= as_global(bs.redo)[0]) break;
            b = as_global(bs.redo)[REDO_LIST + b];
        } else if (b >= nBatches) {
            break;
        }
        const int row = batchRows[(size_t)b * LB + l];
        const int src = row >= 0 ? g.attached[row] : -1;
        if (gid == 0) laneRow[l] = row;
        if constexpr (P::round_arrays) D = as_global(bs.D + (size_t)b * SE);
        if constexpr (P::has_labels_in_bs) LBL = as_global(bs.LB + (size_t)b * SE);
        // predecessor filter (split kernels): the batch's in-arc flags, one
        // bit per in-arc slot -- the relax sets bit outToIn[a] when some active
        // lane's pre-check of arc a finds dist[u] + w <= dist[x] (every arc
        // that is tight, or violated, in the final state: DESIGN.md §5), the
        // on-demand predecessor pass gathers the flagged in-arcs only.  The
        // relax keeps the bits in LDS behind the pending bitmaps (hitLds: they
        // fit) and writes them out once, at the end of the batch, with bit 1
        // of the batch's flag word; without that bit the pass reads every
        // in-arc.  (Flag stores to HBM from the relax loop cost it three times
        // what the pass gains: DESIGN.md §7.)
        uint32_t* AHw = nullptr;
        if constexpr (P::round_arrays)
            if (bs.arcHit) AHw = as_global(bs.arcHit) + (size_t)b * (size_t)(bs.mStride >> 5);
        uint32_t* const hb = reinterpret_cast<uint32_t*>(smem + BCTRL_BYTES + 8 * nwp);
        const bool hits = HITS && AHw != nullptr && bs.hitLds != 0;
        // ---- init: dist = +inf (clean) for all (v, lane); pending sets empty ----
        {
            ulonglong2* D2 = reinterpret_cast<ulonglong2*>(D);
            const size_t cnt2 = NE / 2;
            const ulonglong2 inf2 = make_ulonglong2(INF_ENC, INF_ENC);
            if constexpr (P::relaxes) {
                for (size_t i = tid; i < cnt2; i += NT) D2[i] = inf2;
                if (hits) {     // no in-arc flagged yet (mStride is a multiple of 128 bits)
                    uint4* const H4 = reinterpret_cast<uint4*>(hb);
                    const int cnt16 = (int)(bs.mStride >> 7);
                    for (int i = tid; i < cnt16; i += NT) H4[i] = make_uint4(0u, 0u, 0u, 0u);
                }
            }
            if constexpr (P::uses_bitmaps)
                for (int w = tid; w < nwp; w += NT) { any0.st(w, 0u); any1.st(w, 0u); }
            if (tid == 0) {
                ctl->qtail = 0;
                ctl->qhead = 0;
                ctl->farAny = 0;
                ctl->farMin = INF_BITS;
                ctl->ambMask = 0u;
                ctl->changed = 0;
                ctl->htail = 0;
                ctl->busyMax = 0;
                ctl->busySum = 0;
                ctl->maxOff = 0.0;
                ctl->dProcs = ctl->dArcs = ctl->dLanes = 0u;
                ctl->dWhy = 0u;
                ctl->dClaim = ctl->dGath = 0u;
            }
        }
        fence_wg();
        __syncthreads();
        // lane offset: how far the source sits ahead of its batch mates (host
        // plan, lane_offsets); key = dist + (maxOff - off) lines the lanes up
        const double off = row >= 0 ? as_global(bs.laneOff)[(size_t)b * LB + l] : 0.0;
        if (gid == 0) atomicMax(reinterpret_cast<unsigned long long*>(&ctl->maxOff), d2b(off));
        if (P::relaxes && gid == 0 && src >= 0) {
            D[(size_t)src * LB + l] = enc_dirty(d2b(0.0));
            any0.set(src);
        }
        fence_wg();
        __syncthreads();
        const double sh = uni(ctl->maxOff) - off;      // >= 0: keys are non-negative

        // ================= 1. delta-stepping over the batch =================
        // Pending state is one bit per VERTEX (LDS) in two sets: NEAR (some
        // lane of u has a dirty value below the bound) and FAR (a dirty value
        // at or above it).  A phase lists and clears the near set and
        // processes each listed vertex: its dirty lanes below the bound are
        // marked clean (CAS on the value read) and relaxed, its dirty lanes
        // at or above the bound send it to the far set.  Clean lanes are
        // never re-relaxed (their value already reached every out-neighbour),
        // so a vertex costs arc traffic only when a lane has a new value.
        // When the near set is empty the bound moves to the bucket of the
        // smallest far key and the far set becomes the near set.
        // Improvements are no-return atomic mins at workgroup scope on the
        // encoding (the line was just read for the pre-check, so the atomic
        // resolves in L2, and no update is lost).  The Bellman check of pass
        // 2 stays as the safety net.
        if (dbg && tid == 0) ctl->t0 = (long long)clock64();
        int par = 0, phases = 0, repairs = 0;
        bool failed = false;
        const int phaseCap = 8 * n + 1024;
        double bound = delta;
        unsigned long long myFar = INF_BITS;      // smallest far key this thread added
        if constexpr (P::reads_relax_flags) failed = (as_global(bs.flags)[b] & 1) != 0;
#ifdef SHDPE_DIAG_WHY
        uint32_t why = failed ? 128u : 0u;
        __shared__ int sDiagViol;
        if (tid == 0) sDiagViol = 0;
        __syncthreads();
#endif
        uint32_t needMask = 0u;
        bool lastFull = true;     // the final attempt ran the full predecessor pass
        // (the redo launch starts at the full pass: what attempt 1 does)
        for (int attempt = PART == 2 && bs.redoRun ? 1 : 0;; ++attempt) {
            const bool fullPred = P::relaxes || (!P::has_labels_in_bs && attempt > 0);
            if (attempt > 0) DIAG_WHY(64u);
            if (attempt > 0) {
                if (tid == 0) {
                    ctl->qtail = 0;
                    ctl->changed = 0;
                    ctl->ambMask = 0u;
                }
                fence_wg();
                __syncthreads();
            }
            for (;;) {   // phases + verification until the Bellman check holds
                if constexpr (P::relaxes) {
                    for (;;) {
                        if (failed) break;
                        const Bits<GB> anyC = par ? any1 : any0;   // near
                        const Bits<GB> anyF = par ? any0 : any1;   // far
                        list_near<NT>(anyC, g.heavyBits, ctl, Q, NS, nw, tid);
                        if (myFar != INF_BITS) {
                            atomicMin(&ctl->farMin, myFar);
                            myFar = INF_BITS;
                        }
                        fence_wg();
                        __syncthreads();
                        const int qn = uni(ctl->qtail);
                        const int hn = uni(ctl->htail);
                        if (qn == 0 && hn == 0) {
                            // bucket settled: advance to the far set, or done
                            const int farAny = uni(ctl->farAny);
                            const double fm = uni(b2d(ctl->farMin));
                            __syncthreads();
                            if (!farAny) break;
                            bound = uni(fm < b2d(INF_BITS) ? bucket_bound(fm, delta) : b2d(INF_BITS));
                            if (tid == 0) {
                                ctl->farAny = 0;
                                ctl->farMin = INF_BITS;
                            }
                            par ^= 1;
                            ++phases;
                            __syncthreads();
                            continue;
                        }
                        if (phases > phaseCap) {        // safety net: never spin the GPU
                            failed = true;
                            break;
                        }
                        int farAdd = 0;
                        const long long tg0 = dbg ? (long long)clock64() : 0;
                        // hubs first (their improvements reach the light vertices in this
                        // phase): one wave per hub, its 64 / LB groups interleave the arcs
                        {
                            constexpr int GPW = 64 / LB;
                            const int wv = tid >> 6, NW = NT >> 6, gw = (tid & 63) / LB;
                            for (int h = wv; h < hn; h += NW) {
                                const int u = ld_wg(&Q[NS - 1 - h]);
                                unsigned long long* const pu = &D[(size_t)u * LB + l];
                                const unsigned long long e0 = ld_d(pu);
                                const int a0 = g.rowPtr[u], a1 = g.rowPtr[u + 1];
                                const double k0 = b2d(dec(e0)) + sh;
                                const bool dirty = is_dirty(e0);
                                const bool below = dirty && k0 < bound;
                                const bool act = EAGER ? dirty && __ballot(below) >> gbase & LBMASK : below;
                                const bool defer = dirty && !act;
                                const uint32_t amask = (uint32_t)(__ballot(act) >> gbase) & LBMASK;
                                const uint32_t dmask = (uint32_t)(__ballot(defer) >> gbase) & LBMASK;
                                if (gw == 0 && l == 0 && dmask) anyF.set(u);
                                if (gw == 0 && defer) {
                                    myFar = d2b(k0) < myFar ? d2b(k0) : myFar;
                                    farAdd = 1;
                                }
                                if (gw == 0 && act) mark_clean(pu, e0);
                                const unsigned long long dub1 = act ? dec(e0) : INF_BITS;
                                if (!__ballot(amask != 0)) continue;       // wave-uniform
                                if (dbg && gw == 0 && l == 0) {
                                    atomicAdd(&ctl->dProcs, 1u);
                                    atomicAdd(&ctl->dArcs, (unsigned int)(a1 - a0));
                                    atomicAdd(&ctl->dLanes, (unsigned int)__popc(amask));
                                }
                                for (int t = a0 + gw * BK; t < a1; t += GPW * BK) {
                                    int xs[BK], rs[BK];
                                    double ws[BK];
                                    unsigned long long dx[BK];
#pragma unroll
                                    for (int k = 0; k < BK; ++k) {
                                        const int a = t + k;
                                        const bool ok = a < a1;
                                        const Arc A = g.arcs[ok ? a : 0];
                                        xs[k] = ok ? A.col : -1;
                                        ws[k] = A.lat;
                                        rs[k] = A.pad;
                                    }
#pragma unroll
                                    for (int k = 0; k < BK; ++k)
                                        dx[k] = relax_ld(D, xs[k] >= 0 ? xs[k] : 0, LB, l);
#pragma unroll
                                    for (int k = 0; k < BK; ++k) {
                                        const int x = xs[k];
                                        bool impN = false, impF = false, hit = false;
                                        if (x >= 0) {
                                            const double nd = b2d(dub1) + ws[k];
                                            const unsigned long long nb = d2b(nd);
                                            hit = act && nb <= dec(dx[k]);
                                            if (nb < dec(dx[k])) {
                                                relax_min(&D[(size_t)x * LB + l], enc_dirty(nb));
                                                const double kx = nd + sh;
                                                impN = kx < bound;
                                                impF = !impN;
                                                if (impF) myFar = d2b(kx) < myFar ? d2b(kx) : myFar;
                                            }
                                        }
                                        const uint64_t bn = __ballot(impN), bf = __ballot(impF);
                                        uint64_t bh = 0;
                                        if constexpr (HITS) bh = __ballot(hit);
                                        if (l == 0) {
                                            if ((bn >> gbase) & LBMASK) anyC.set(x);
                                            if ((bf >> gbase) & LBMASK) {
                                                anyF.set(x);
                                                farAdd = 1;
                                            }
                                            // tight or improving in some lane: flag the in-arc
                                            if constexpr (HITS)
                                                if (hits && ((bh >> gbase) & LBMASK)) atomicOr(&hb[rs[k] >> 5], 1u << (rs[k] & 31));
                                        }
                                    }
                                }
                            }
                        }
                        // Groups take BV queue entries at a time from an LDS counter, so
                        // the phase ends when the last entry is done rather than when the
                        // unluckiest static share is.  A value loaded ahead may be stale;
                        // like any racing read it is only ever larger (entries decrease):
                        // relaxing from it is wasted work, and its clean mark (atomic min)
                        // leaves a newer dirty value dirty for the next listing round.
                        const int qc = qn > 0 ? qn - 1 : 0;
                        auto take = [&]() {
                            int i = 0;
                            if (l == 0) i = atomicAdd(&ctl->qhead, BV);
                            return __shfl(i, gbase, 64);
                        };
                        // A three-stage software pipeline over the group's takes (BV
                        // vertices each).  The group's lanes hold ONE arc record per
                        // vertex (lane l: arc a0 + l of the vertex's first LB arcs --
                        // one coalesced LB x 16-B read per group instead of BK
                        // broadcast records per round and a dependent record round
                        // trip before every dist gather); the relaxing lanes take the
                        // heads by cross-lane reads.  Per take the group issues the
                        // records of the next take, the dist lines + row ranges of the
                        // one after, and the queue entries of the third, then relaxes
                        // the current vertices: their chain is the BKR-wide dist
                        // gathers only.  An entry past the queue end is u = -1 (takes
                        // rise monotonically, so a take whose first entry is -1 ends).
                        auto q_at = [&](int i) { return i < qn ? ld_wg(&Q[min(i, qc)]) : -1; };
                        auto ld_head = [&](int uu, unsigned long long& d, int& r0, int& r1) {
                            const int uc = uu >= 0 ? uu : 0;
                            const unsigned long long d0 = ld_d(&D[(size_t)uc * LB + l]);
                            const int x0 = g.rowPtr[uc], x1 = g.rowPtr[uc + 1];
                            d = uu >= 0 ? d0 : INF_ENC;
                            r0 = uu >= 0 ? x0 : 0;
                            r1 = uu >= 0 ? x1 : 0;
                        };
                        auto ld_arc = [&](int a, int aEnd, int& c, double& w, int& r) {
                            const bool ok = a < aEnd;
                            const Arc A = g.arcs[ok ? a : 0];
                            c = ok ? A.col : -1;
                            w = A.lat;
                            r = A.pad;      // the arc's slot in its head's in-list (same 16-B record)
                        };
                        int uC[BV], u1[BV], u2[BV], a0C[BV], a1C[BV], a01[BV], a11[BV], mcC[BV], mrC[BV];
                        unsigned long long dbC[BV], db1[BV];
                        double mlC[BV];
                        {
                            const int i0 = take(), i1 = take(), i2 = take();
#pragma unroll
                            for (int v = 0; v < BV; ++v) {
                                uC[v] = q_at(i0 + v);
                                u1[v] = q_at(i1 + v);
                                u2[v] = q_at(i2 + v);
                            }
                        }
#pragma unroll
                        for (int v = 0; v < BV; ++v) {
                            ld_head(uC[v], dbC[v], a0C[v], a1C[v]);
                            ld_head(u1[v], db1[v], a01[v], a11[v]);
                        }
#pragma unroll
                        for (int v = 0; v < BV; ++v) ld_arc(a0C[v] + l, a1C[v], mcC[v], mlC[v], mrC[v]);
                        while (uC[0] >= 0) {
                            int mc1[BV], mr1[BV], a02[BV], a12[BV], u3[BV];
                            double ml1[BV];
                            unsigned long long db2[BV];
#pragma unroll
                            for (int v = 0; v < BV; ++v) ld_arc(a01[v] + l, a11[v], mc1[v], ml1[v], mr1[v]);
#pragma unroll
                            for (int v = 0; v < BV; ++v) ld_head(u2[v], db2[v], a02[v], a12[v]);
                            {
                                const int i3 = take();
#pragma unroll
                                for (int v = 0; v < BV; ++v) u3[v] = q_at(i3 + v);
                            }
                            unsigned long long dub[BV];
                            int deg[BV], maxd = 0;
#pragma unroll
                            for (int v = 0; v < BV; ++v) {
                                const double k0 = b2d(dec(dbC[v])) + sh;
                                const bool dirty = is_dirty(dbC[v]);
                                const bool below = dirty && k0 < bound;
                                const bool act = EAGER ? dirty && __ballot(below) >> gbase & LBMASK : below;
                                const bool defer = dirty && !act;
                                const uint32_t amask = (uint32_t)(__ballot(act) >> gbase) & LBMASK;
                                const uint32_t dmask = (uint32_t)(__ballot(defer) >> gbase) & LBMASK;
                                if (l == 0 && dmask) anyF.set(uC[v]);
                                if (defer) {
                                    myFar = d2b(k0) < myFar ? d2b(k0) : myFar;
                                    farAdd = 1;
                                }
                                if (act) mark_clean(&D[(size_t)uC[v] * LB + l], dbC[v]);
                                dub[v] = act ? dec(dbC[v]) : INF_BITS;
                                deg[v] = amask ? a1C[v] - a0C[v] : 0;          // group-uniform
                                if (amask && dbg && l == 0) {
                                    atomicAdd(&ctl->dProcs, 1u);
                                    atomicAdd(&ctl->dArcs, (unsigned int)deg[v]);
                                    atomicAdd(&ctl->dLanes, (unsigned int)__popc(amask));
                                }
                                maxd = max(maxd, deg[v]);
                            }
                            // relax the out-arcs for the dirty lanes below the bound
                            for (int c0 = 0; c0 < maxd; c0 += LB) {
                                int mc[BV], mr[BV];
                                double ml[BV];
#pragma unroll
                                for (int v = 0; v < BV; ++v) {
                                    mc[v] = mcC[v];
                                    ml[v] = mlC[v];
                                    mr[v] = mrC[v];
                                    if (c0 > 0) ld_arc(a0C[v] + c0 + l, a0C[v] + deg[v], mc[v], ml[v], mr[v]);   // degree > LB
                                }
                                const int cn = min(LB, maxd - c0);
                                uint32_t hacc[BV];      // the chunk's arcs with a hit in some lane
#pragma unroll
                                for (int v = 0; v < BV; ++v) hacc[v] = 0u;
                                for (int t = 0; t < cn; t += BKR) {
                                    int xs[BV][BKR];
                                    double ws[BV][BKR];
                                    unsigned long long dx[BV][BKR];
#pragma unroll
                                    for (int v = 0; v < BV; ++v)
#pragma unroll
                                        for (int k = 0; k < BKR; ++k) {
                                            const int srcL = gbase + min(t + k, LB - 1);   // inside the group
                                            const int c = __shfl(mc[v], srcL, 64);
                                            ws[v][k] = __shfl(ml[v], srcL, 64);
                                            xs[v][k] = t + k < cn && c0 + t + k < deg[v] ? c : -1;   // (the chunk's own records)
                                        }
#pragma unroll
                                    for (int v = 0; v < BV; ++v)
#pragma unroll
                                        for (int k = 0; k < BKR; ++k)
                                            dx[v][k] = relax_ld(D, xs[v][k] >= 0 ? xs[v][k] : 0, LB, l);
#pragma unroll
                                    for (int v = 0; v < BV; ++v)
#pragma unroll
                                        for (int k = 0; k < BKR; ++k) {
                                            const int x = xs[v][k];
                                            bool impN = false, impF = false, hit = false;
                                            if (x >= 0) {
                                                const double nd = b2d(dub[v]) + ws[v][k];
                                                const unsigned long long nb = d2b(nd);
                                                hit = dub[v] != INF_BITS && nb <= dec(dx[v][k]);
                                                if (nb < dec(dx[v][k])) {
                                                    relax_min(&D[(size_t)x * LB + l], enc_dirty(nb));
                                                    const double kx = nd + sh;
                                                    impN = kx < bound;
                                                    impF = !impN;
                                                    if (impF) myFar = d2b(kx) < myFar ? d2b(kx) : myFar;
                                                }
                                            }
                                            const uint64_t bn = __ballot(impN), bf = __ballot(impF);
                                            if (l == 0) {
                                                if ((bn >> gbase) & LBMASK) anyC.set(x);
                                                if ((bf >> gbase) & LBMASK) {
                                                    anyF.set(x);
                                                    farAdd = 1;
                                                }
                                            }
                                            if constexpr (HITS) {      // (branch-free: `hits` gates the store below)
                                                const uint64_t bh = __ballot(hit);
                                                hacc[v] |= (bh >> gbase) & LBMASK ? 1u << ((t + k) & 31) : 0u;
                                            }
                                        }
                                }
                                // tight or improving in some lane: the lane that holds the
                                // arc's record flags its in-arc slot (once per chunk)
                                if constexpr (HITS) {
#pragma unroll
                                    for (int v = 0; v < BV; ++v)
                                        if (hits && ((hacc[v] >> l) & 1u)) atomicOr(&hb[mr[v] >> 5], 1u << (mr[v] & 31));
                                }
                            }
#pragma unroll
                            for (int v = 0; v < BV; ++v) {
                                uC[v] = u1[v]; dbC[v] = db1[v]; a0C[v] = a01[v]; a1C[v] = a11[v];
                                mcC[v] = mc1[v]; mlC[v] = ml1[v]; mrC[v] = mr1[v];
                                u1[v] = u2[v]; db1[v] = db2[v]; a01[v] = a02[v]; a11[v] = a12[v];
                                u2[v] = u3[v];
                            }
                        }
                        if (dbg && l == 0) {
                            const unsigned long long bz = (unsigned long long)((long long)clock64() - tg0);
                            atomicMax(&ctl->busyMax, bz);
                            atomicAdd(&ctl->busySum, bz);
                        }
                        if (farAdd) ctl->farAny = 1;
                        fence_wg();
                        __syncthreads();
                        if (tid == 0) {
                            ctl->qtail = 0;
                            ctl->qhead = 0;
                            ctl->htail = 0;
                            if (dbg) {
                                atomicAdd(&dbg[16 * b + 12], (int)(ctl->busyMax >> 10));
                                atomicAdd(&dbg[16 * b + 13], (int)((ctl->busySum / NG) >> 10));
                                atomicAdd(&dbg[16 * b + 14], qn);
                                ctl->busyMax = 0;
                                ctl->busySum = 0;
                            }
                        }
                        ++phases;
                        __syncthreads();
                    }
                }   // relaxes
                if (dbg && tid == 0) ctl->t1 = (long long)clock64();
                if constexpr (P::relax_part) break;
                if constexpr (P::label_part) break;      // (the predecessor part ran, PART 5)

                // ================= 2. Bellman check + predecessor pass ===============
                // (a) every entry must satisfy dist[v] <= dist[u] + w for all in-arcs
                //     (a violation = an update lost to a concurrent plain store: fix
                //     it, mark v pending, and go back to phase 1);
                // (b) igraph sets parent[v] from the first POPPED tight predecessor:
                //     the tight in-arc with minimum dist[u]; equal minima from distinct
                //     vertices (or a zero-increment arc) -> the heap decides -> tie
                //     row (k_exact_rows) if such an entry lies on a target's path.
                int viol = 0;
                {
                    const Bits<GB> anyC = par ? any1 : any0;
                    // on demand: vertices are claimed in the (empty) far bitmap and
                    // listed in Q, targets first, then round by round the tree
                    // parents of the last round's entries in every lane
                    const Bits<GB> clm = par ? any0 : any1;
                    // entries of in-degree >= PRED_HEAVY are set aside per round and
                    // scanned by a whole wave each (its groups split the in-arcs and
                    // combine by cross-group shuffles): one group on a hub's ~1000
                    // in-arcs would set the round's length.  List in the LDS beyond
                    // the bitmaps (free until the label walks), capped by that room.
                    int* const heavyList = reinterpret_cast<int*>(smem + BCTRL_BYTES + (GB ? 0 : 8 * nwp));
                    const int stackB = NT * SMAX * 8, bitsB = GB ? 0 : 8 * nwp;
                    const int hcap = P::pred_part ? pred_heavy_cap(nwp, GB) : min(4096, max(0, stackB - bitsB) / 4);
                    int lo = 0, hi = n;
                    // the on-demand pass gathers only the in-arcs the relax flagged (a
                    // superset of the tight ones); the full pass reads every in-arc
                    bool filt = false;
                    if constexpr (P::reads_relax_flags) filt = !fullPred && AHw != nullptr && (as_global(bs.flags)[b] & 2) != 0;
                    if (!fullPred) {
                        for (int j = tid; j < g.T; j += NT) {
                            const int v = g.attached[j];
                            wave_append(Q, &ctl->qtail, !clm.test_set(v), v);
                        }
                        fence_wg();
                        __syncthreads();
                        hi = uni(ctl->qtail);
                        __syncthreads();
                    }
                    while (lo < hi) {
                        // the relax loop's three-stage pipeline (BV list entries per
                        // group and stride): the group's lanes hold one in-arc record
                        // per entry (lane l: in-arc a0 + l, one coalesced read), the
                        // scan takes the tails by cross-lane reads, so an entry's
                        // chain is its BKQ-wide dist gathers.  Records of the next
                        // stride, dist lines + in-arc ranges of the one after, list
                        // entries of the third are in flight meanwhile.
                        const int S = NG * BV;
                        auto item = [&](int i) { return i < hi ? (fullPred ? i : ld_wg(&Q[i])) : -1; };
                        auto ld_head = [&](int vv, unsigned long long& d, int& r0, int& r1) {
                            const int vc = vv >= 0 ? vv : 0;
                            const unsigned long long d0 = dec(ld_wg(&D[(size_t)vc * LB + l]));
                            const int x0 = undirected ? g.rowPtr[vc] : g.inPtr[vc];
                            const int x1 = undirected ? g.rowPtr[vc + 1] : g.inPtr[vc + 1];
                            d = vv >= 0 ? d0 : INF_BITS;
                            r0 = vv >= 0 ? x0 : 0;
                            r1 = vv >= 0 ? x1 : 0;
                        };
                        // (filtered pass: an in-arc the relax did not flag reads as absent
                        // -- its flag bit is loaded beside its record, one or two words
                        // per group)
                        auto ld_rec = [&](int a, int aEnd, int& c, double& w) {
                            bool ok = a < aEnd;
                            const int ac = ok ? a : 0;
                            if (filt) ok = ok && ((AHw[ac >> 5] >> (ac & 31)) & 1u) != 0;
                            if (undirected) {
                                const Arc A = g.arcs[ac];
                                c = A.col;
                                w = A.lat;
                            } else {
                                c = g.inCol[ac];
                                w = g.inLat[ac];
                            }
                            c = ok ? c : -1;
                        };
                        int v0 = lo + gid * BV;
                        int vC[BV], v1[BV], v2[BV], a0C[BV], a1C[BV], a01[BV], a11[BV], mcC[BV];
                        unsigned long long dC[BV], d1[BV];
                        double mlC[BV];
#pragma unroll
                        for (int v = 0; v < BV; ++v) {
                            vC[v] = item(v0 + v);
                            v1[v] = item(v0 + S + v);
                            v2[v] = item(v0 + 2 * S + v);
                        }
#pragma unroll
                        for (int v = 0; v < BV; ++v) {
                            ld_head(vC[v], dC[v], a0C[v], a1C[v]);
                            ld_head(v1[v], d1[v], a01[v], a11[v]);
                        }
#pragma unroll
                        for (int v = 0; v < BV; ++v) ld_rec(a0C[v] + l, a1C[v], mcC[v], mlC[v]);
                        for (; v0 < hi; v0 += S) {
                            int mc1[BV], a02[BV], a12[BV], v3[BV];
                            double ml1[BV];
                            unsigned long long d2[BV];
#pragma unroll
                            for (int v = 0; v < BV; ++v) ld_rec(a01[v] + l, a11[v], mc1[v], ml1[v]);
#pragma unroll
                            for (int v = 0; v < BV; ++v) ld_head(v2[v], d2[v], a02[v], a12[v]);
#pragma unroll
                            for (int v = 0; v < BV; ++v) v3[v] = item(v0 + 3 * S + v);
                            bool root[BV], hvy[BV];
                            unsigned long long best[BV], mn[BV];
                            int cnt[BV], ba[BV], bu[BV], deg[BV], maxd = 0;
#pragma unroll
                            for (int v = 0; v < BV; ++v) {
                                root[v] = vC[v] == src || src < 0;
                                best[v] = INF_BITS;
                                mn[v] = INF_BITS;
                                cnt[v] = 0;
                                ba[v] = -1;
                                bu[v] = -1;
                                deg[v] = vC[v] >= 0 ? a1C[v] - a0C[v] : 0;   // group-uniform
                                hvy[v] = false;
                                if (dbg && !fullPred && l == 0 && deg[v]) atomicAdd(&ctl->dClaim, (unsigned int)deg[v]);
                                if (deg[v] >= PRED_HEAVY) {                   // -> the round's wave pass
                                    int slot = 0;
                                    if (l == 0) slot = atomicAdd(&ctl->htail, 1);
                                    slot = __shfl(slot, gbase, 64);
                                    if (slot < hcap) {
                                        if (l == 0) heavyList[slot] = vC[v];
                                        hvy[v] = true;
                                        deg[v] = 0;
                                    }
                                }
                                maxd = max(maxd, deg[v]);
                            }
                            for (int c0 = 0; c0 < maxd; c0 += LB) {
                                int mc[BV];
                                double ml[BV];
#pragma unroll
                                for (int v = 0; v < BV; ++v) {
                                    mc[v] = mcC[v];
                                    ml[v] = mlC[v];
                                    if (c0 > 0) ld_rec(a0C[v] + c0 + l, a0C[v] + deg[v], mc[v], ml[v]);
                                }
                                // the chunk's records to gather: those present (in the
                                // filtered pass, flagged), as a mask over the group's lanes;
                                // the gather rounds walk its set bits in in-list order
                                uint32_t hm[BV], hany = 0u;
#pragma unroll
                                for (int v = 0; v < BV; ++v) {
                                    const int rem = deg[v] - c0;
                                    const uint32_t dm = rem >= LB ? LBMASK : rem > 0 ? (1u << (rem & 31)) - 1u : 0u;
                                    hm[v] = (uint32_t)(__ballot(mc[v] >= 0) >> gbase) & dm;
                                    if (dbg && !fullPred && l == 0 && hm[v]) atomicAdd(&ctl->dGath, (unsigned int)__popc(hm[v]));
                                    hany |= hm[v];
                                }
                                while (hany) {
                                    int cu[BV][BKQ], jj[BV][BKQ];
                                    double lw[BV][BKQ];
                                    unsigned long long du[BV][BKQ];
                                    hany = 0u;
#pragma unroll
                                    for (int v = 0; v < BV; ++v) {
#pragma unroll
                                        for (int k = 0; k < BKQ; ++k) {
                                            const bool on = hm[v] != 0u;
                                            const int j = on ? __ffs(hm[v]) - 1 : 0;
                                            hm[v] &= hm[v] - 1u;
                                            const int srcL = gbase + j;
                                            const int c = __shfl(mc[v], srcL, 64);
                                            lw[v][k] = __shfl(ml[v], srcL, 64);
                                            cu[v][k] = on ? c : -1;   // (a repeat would count as a tie)
                                            jj[v][k] = j;
                                        }
                                        hany |= hm[v];
                                    }
#pragma unroll
                                    for (int v = 0; v < BV; ++v)
#pragma unroll
                                        for (int k = 0; k < BKQ; ++k) {
                                            const unsigned long long t2 =
                                                dec(ld_wg(&D[(size_t)(cu[v][k] >= 0 ? cu[v][k] : 0) * LB + l]));
                                            du[v][k] = cu[v][k] >= 0 ? t2 : INF_BITS;
                                        }
#pragma unroll
                                    for (int v = 0; v < BV; ++v)
#pragma unroll
                                        for (int k = 0; k < BKQ; ++k) {
                                            if (cu[v][k] < 0 || root[v]) continue;
                                            const double cand = b2d(du[v][k]) + lw[v][k];
                                            const unsigned long long cb = d2b(cand);
                                            mn[v] = cb < mn[v] ? cb : mn[v];
                                            if (dC[v] != INF_BITS && du[v][k] <= dC[v] && cand == b2d(dC[v])) {
                                                if (du[v][k] < best[v]) {
                                                    best[v] = du[v][k];
                                                    cnt[v] = 1;
                                                    ba[v] = a0C[v] + c0 + jj[v][k];
                                                    bu[v] = cu[v][k];
                                                } else if (du[v][k] == best[v]) {
                                                    ++cnt[v];
                                                }
                                            }
                                        }
                                }
                            }
#pragma unroll
                            for (int v = 0; v < BV; ++v) {
                                const int vv = vC[v];
                                if (vv < 0 || hvy[v]) continue;
                                const size_t e = (size_t)vv * LB + l;
                                const bool bad = !root[v] && mn[v] < dC[v];
                                if (bad) {
                                    D[e] = enc_dirty(mn[v]);
                                    viol = 1;
                                    DIAG_VIOL(b, vv, l, dC[v], mn[v], 0);
                                }
                                const uint32_t bm = (uint32_t)(__ballot(bad) >> gbase) & LBMASK;
                                if (bm && l == 0) anyC.set(vv);
                                const bool tree = !root[v] && dC[v] != INF_BITS && ba[v] >= 0;
                                // ambiguous (see the generic loop below)
                                const bool ea = !root[v] && dC[v] != INF_BITS && (cnt[v] != 1 || best[v] == dC[v]);
                                const int hx = tree ? ba[v] : -1;
                                const bool isSrc = vv == src;
                                lbl_st(&LBL[e], isSrc ? 1.0 : -1.0, isSrc ? 0 : -1,
                                       ea ? (TIE_AMB | (hx > 0 ? hx : 0)) : hx);
                                if (!tree) bu[v] = -1;
                            }
                            if (!fullPred) {
#pragma unroll
                                for (int v = 0; v < BV; ++v) {
                                    const int p = vC[v] >= 0 && !hvy[v] ? bu[v] : -1;
                                    wave_append(Q, &ctl->qtail, p >= 0 && !clm.test_set(p), p);
                                }
                            }
#pragma unroll
                            for (int v = 0; v < BV; ++v) {
                                vC[v] = v1[v]; dC[v] = d1[v]; a0C[v] = a01[v]; a1C[v] = a11[v];
                                mcC[v] = mc1[v]; mlC[v] = ml1[v];
                                v1[v] = v2[v]; d1[v] = d2[v]; a01[v] = a02[v]; a11[v] = a12[v];
                                v2[v] = v3[v];
                            }
                        }
                        {
                            // the round's heavy entries, one wave each
                            fence_wg();
                            __syncthreads();
                            const int nh = min(uni(ctl->htail), hcap);
                            constexpr int GPW = 64 / LB;
                            const int wv = tid >> 6, NW = NT >> 6, gw = (tid & 63) / LB;
                            for (int h = wv; h < nh; h += NW) {
                                const int vv = __builtin_amdgcn_readfirstlane(ld_wg(&heavyList[h]));
                                const unsigned long long dv = dec(ld_wg(&D[(size_t)vv * LB + l]));
                                const int a0 = undirected ? g.rowPtr[vv] : g.inPtr[vv];
                                const int a1 = undirected ? g.rowPtr[vv + 1] : g.inPtr[vv + 1];
                                const int deg = a1 - a0;
                                const bool root = vv == src || src < 0;
                                unsigned long long best = INF_BITS, mn = INF_BITS;
                                int cnt = 0, ba = -1, bu = -1;
                                for (int c0 = gw * LB; c0 < deg; c0 += GPW * LB) {
                                    int mc;
                                    double ml;
                                    {
                                        const int a = a0 + c0 + l;
                                        bool ok = a < a1;
                                        const int ac = ok ? a : 0;
                                        if (filt) ok = ok && ((AHw[ac >> 5] >> (ac & 31)) & 1u) != 0;
                                        if (undirected) {
                                            const Arc A = g.arcs[ac];
                                            mc = A.col;
                                            ml = A.lat;
                                        } else {
                                            mc = g.inCol[ac];
                                            ml = g.inLat[ac];
                                        }
                                        mc = ok ? mc : -1;
                                    }
                                    // (the same mask walk as the groups' scan, per wave chunk)
                                    uint32_t hm = (uint32_t)(__ballot(mc >= 0) >> gbase) & LBMASK;
                                    if (dbg && !fullPred && l == 0 && hm) atomicAdd(&ctl->dGath, (unsigned int)__popc(hm));
                                    while (hm) {
                                        int cu[BKQ], jj[BKQ];
                                        double lw[BKQ];
                                        unsigned long long du[BKQ];
#pragma unroll
                                        for (int k = 0; k < BKQ; ++k) {
                                            const bool on = hm != 0u;
                                            const int j = on ? __ffs(hm) - 1 : 0;
                                            hm &= hm - 1u;
                                            const int srcL = gbase + j;
                                            const int c = __shfl(mc, srcL, 64);
                                            lw[k] = __shfl(ml, srcL, 64);
                                            cu[k] = on ? c : -1;
                                            jj[k] = j;
                                        }
#pragma unroll
                                        for (int k = 0; k < BKQ; ++k) {
                                            const unsigned long long t2 =
                                                dec(ld_wg(&D[(size_t)(cu[k] >= 0 ? cu[k] : 0) * LB + l]));
                                            du[k] = cu[k] >= 0 ? t2 : INF_BITS;
                                        }
#pragma unroll
                                        for (int k = 0; k < BKQ; ++k) {
                                            if (cu[k] < 0 || root) continue;
                                            const double cand = b2d(du[k]) + lw[k];
                                            const unsigned long long cb = d2b(cand);
                                            mn = cb < mn ? cb : mn;
                                            if (dv != INF_BITS && du[k] <= dv && cand == b2d(dv)) {
                                                if (du[k] < best) {
                                                    best = du[k];
                                                    cnt = 1;
                                                    ba = a0 + c0 + jj[k];
                                                    bu = cu[k];
                                                } else if (du[k] == best) {
                                                    ++cnt;
                                                }
                                            }
                                        }
                                    }
                                }
                                // combine the groups' scans (lane l of every group holds
                                // source l): counts of equal minima add up, so an entry is
                                // ambiguous exactly as after one sequential scan
                                for (int o = LB; o < 64; o <<= 1) {
                                    const unsigned long long ob = __shfl_xor(best, o, 64), om = __shfl_xor(mn, o, 64);
                                    const int oc = __shfl_xor(cnt, o, 64), oa = __shfl_xor(ba, o, 64), ou = __shfl_xor(bu, o, 64);
                                    mn = om < mn ? om : mn;
                                    if (ob < best) {
                                        best = ob; cnt = oc; ba = oa; bu = ou;
                                    } else if (ob == best && ob != INF_BITS) {
                                        cnt += oc;
                                        if (oa >= 0 && (ba < 0 || oa < ba)) { ba = oa; bu = ou; }
                                    }
                                }
                                const size_t e = (size_t)vv * LB + l;
                                const bool bad = !root && mn < dv;
                                if (bad && gw == 0) {
                                    D[e] = enc_dirty(mn);
                                    viol = 1;
                                    DIAG_VIOL(b, vv, l, dv, mn, 1);
                                }
                                const uint32_t bm = (uint32_t)(__ballot(bad) >> gbase) & LBMASK;
                                if (bm && l == 0 && gw == 0) anyC.set(vv);
                                const bool tree = !root && dv != INF_BITS && ba >= 0;
                                const bool ea = !root && dv != INF_BITS && (cnt != 1 || best == dv);
                                const int hx = tree ? ba : -1;
                                if (gw == 0) {
                                    const bool isSrc = vv == src;
                                    lbl_st(&LBL[e], isSrc ? 1.0 : -1.0, isSrc ? 0 : -1,
                                           ea ? (TIE_AMB | (hx > 0 ? hx : 0)) : hx);
                                }
                                if (!fullPred) {
                                    const int p = tree ? bu : -1;
                                    wave_append(Q, &ctl->qtail, gw == 0 && p >= 0 && !clm.test_set(p), p);
                                }
                            }
                            fence_wg();
                            __syncthreads();
                            if (tid == 0) ctl->htail = 0;   // (every thread read it before the barrier)
                        }
                        if (fullPred) break;
                        fence_wg();
                        __syncthreads();
                        lo = hi;
                        hi = uni(ctl->qtail);
                        __syncthreads();
                    }
                    if (!fullPred) {
                        for (int w = tid; w < nwp; w += NT) clm.st(w, 0u);
                        if (tid == 0) ctl->qtail = 0;
                    }
                }
                if (viol) ctl->changed = 1;
                if (viol) DIAG_WHY(attempt ? 4u : 2u);
                fence_wg();
                __syncthreads();
                const int anyViol = uni(ctl->changed);
                __syncthreads();
                if (tid == 0) {
                    ctl->changed = 0;
                    ctl->ambMask = 0u;
                }
                __syncthreads();
                if (!anyViol || failed) break;
                if constexpr (!P::relaxes) {   // no relaxation here to repair with: exact path
                    failed = true;
                    break;
                }
                ++repairs;
            }   // verification loop
            if constexpr (P::relax_part) {
                if constexpr (HITS)
                    if (hits) flush_hits<NT>(hb, AHw, bs.mStride, tid);
                if (tid == 0) as_global(bs.flags)[b] = (failed ? 1 : 0) | (hits ? 2 : 0);
                break;
            }
            if (dbg && tid == 0) ctl->t2 = (long long)clock64();
            if constexpr (P::pred_part) {
                // the one value that crosses to the label part: a violation fails the batch
                if (tid == 0 && failed) as_global(bs.flags)[b] |= 1;
                break;
            }

            // ================= 3. labels on demand + row writer ==================
            // Only entries on some target's path need hops and reliability (27%
            // of the entries at C4).  Each lane resolves a target by walking its
            // predecessor chain up to the first entry with known labels (at the
            // latest the source: hops 0, rel 1) and unwinding the walk:
            // hops[x] = hops[p] + 1, rel[x] = rel[p] * r(p, x) -- the reference's
            // left fold (topology.c:1430, :1499) in path order, exactly.  Unwound
            // entries keep their labels for later walks of the same lane; each
            // label is written once with the only value the fold can give, so a
            // racing reader sees a complete pair (H >= 0 and R >= 0) or an
            // unresolved entry and walks on.  The walk stack holds SMAX
            // (entry, arc) pairs per thread in LDS (the relax bitmaps are dead);
            // a longer chain is resolved from the top, SMAX levels at a time.
            // An ambiguous entry (TIE_AMB) on a walked chain makes the row a tie
            // row; ambiguous entries off every target path never matter.  Very
            // deep trees (a walk over WALK_BUDGET steps: restarts cost
            // O(depth^2 / SMAX)) switch to Gauss-Seidel sweeps over all entries
            // and a second writer pass.
            // latency floor: the lane's own source must sit at distance exactly 0
            // in the array its row is written from (latencies are > 0, so only
            // the source is) -- an array that is not this lane's sends the row to
            // the exact kernel, never to the table
            uint32_t relAmb = row >= 0 && dec(ld_wg(&D[(size_t)(src >= 0 ? src : 0) * LB + l])) != 0ull ? 1u : 0u;
            bool retry = false;
            for (int pass = 0; pass < 2; ++pass) {
                bool deep = false;
                if (!failed && row >= 0) {
                    int2* const stk = reinterpret_cast<int2*>(smem + BCTRL_BYTES);
                    const int T = (int)tab.T;
                    // pass 0: the deep-tree budget; pass 1: only the never-spin net
                    // (every consistent entry is resolved by then)
                    // (32-bit: the [v][LB] entry indices below are 32-bit already)
                    const int stepCap = pass == 0 ? WALK_BUDGET : 4 * n + 64;
                    for (int j = gid; j < T; j += NG) {
                        const int t = g.attached[j];
                        if (t != src) {
                            const size_t e = (size_t)t * LB + l;
                            const unsigned long long dt = dec(ld_wg(&D[(size_t)t * LB + l]));
                            if (dt != INF_BITS) {
                                // one record per step: an entry's record holds its
                                // parent arc, the parent's record its labels and the
                                // next arc up
                                Lbl cr = lbl_ld(&LBL[e]);
                                int steps = 0;
                                int cur = (int)e;
                                while (!lbl_known(cr)) {
                                    int sp = 0, x = cur, hp = 0;
                                    Lbl xr = cr;
                                    double rp = 0.0;
                                    bool found = false;
                                    while (sp < SMAX) {
                                        const int a = xr.arc;
                                        if (a < 0 || ++steps > stepCap) {
                                            if (a >= 0 && pass == 0) deep = true;   // -> sweeps
                                            else { relAmb = 1u; DIAG_WHY(8u); }   // no parent / a cycle: exact path
                                            sp = 0;
                                            found = true;
                                            break;
                                        }
                                        relAmb |= (uint32_t)((a & TIE_AMB) != 0);
                                        if (a & TIE_AMB) DIAG_WHY(16u);
                                        stk[sp * NT + tid] = make_int2(x, a);
                                        ++sp;
                                        const int pe = g.inCol[a & ~TIE_AMB] * LB + l;
                                        const Lbl pr = lbl_ld(&LBL[pe]);
                                        if (lbl_known(pr)) {
                                            hp = pr.hops;
                                            rp = pr.rel;
                                            found = true;
                                            break;
                                        }
                                        x = pe;
                                        xr = pr;
                                    }
                                    if (!found) {           // chain longer than SMAX: its top first
                                        cur = x;
                                        cr = xr;
                                        continue;
                                    }
                                    for (int i = sp - 1; i >= 0; --i) {
                                        const int2 sx = stk[i * NT + tid];
                                        hp += 1;
                                        rp = rp * g.inRel[sx.y & ~TIE_AMB];
                                        lbl_st(&LBL[sx.x], rp, hp, sx.y);
                                    }
                                    if (sp == 0) break;     // gave up (deep / inconsistent)
                                    if (cur == (int)e) break;
                                    cur = (int)e;           // top segment resolved: walk again
                                    cr = lbl_ld(&LBL[e]);
                                }
                            }
                        }
                    }
                }
                if (deep) ctl->changed = 1;
                if (deep) DIAG_WHY(32u);
                fence_wg();
                __syncthreads();
                const int anyDeep = uni(ctl->changed);
                __syncthreads();
                if (tid == 0) ctl->changed = 0;
                __syncthreads();
                if (!anyDeep) break;
                if (!fullPred) {         // the sweeps read every entry's parent
                    retry = true;
                    break;
                }
                // Gauss-Seidel: every tree entry whose parent has labels takes them
                // (+1, * r) until a sweep changes nothing (<= depth sweeps).  These
                // entries were not walked, so an ambiguous one sends its row to the
                // exact path (conservative).  Cycles of zero-increment parents stay
                // unresolved and the second pass's walks flag them.
                for (int sweep = 0; sweep <= n + 1; ++sweep) {
                    int ch = 0;
                    for (size_t e = tid; e < NE; e += NT) {
                        const Lbl er = lbl_ld(&LBL[e]);
                        const int a = er.arc;
                        if (a < 0) continue;
                        const int ll = (int)(e % LB);
                        const int arc = a & ~TIE_AMB;
                        const int pe = g.inCol[arc] * LB + ll;
                        const Lbl pr = lbl_ld(&LBL[pe]);
                        if (!lbl_known(pr)) continue;
                        const int hn = pr.hops + 1;
                        const double rn = pr.rel * g.inRel[arc];
                        if (er.hops != hn || er.rel != rn) {
                            lbl_st(&LBL[e], rn, hn, a);
                            ch = 1;
                            if (a & TIE_AMB) atomicOr(&ctl->ambMask, 1u << ll);
                        }
                    }
                    if (ch) ctl->changed = 1;
                    fence_wg();
                    __syncthreads();
                    const int any = uni(ctl->changed);
                    __syncthreads();
                    if (tid == 0) ctl->changed = 0;
                    __syncthreads();
                    if (!any) break;
                }
            }   // label passes
            if (dbg && tid == 0) dbg[16 * b + 2] = (int)(((long long)clock64() - ctl->t2) >> 10);   // walks
            // ---- row writer: the lanes' rows are written target block by
            // target block through an LDS tile (the walk stacks' space): a
            // group holds one target of 16 rows, so direct stores would scatter
            // 16 rows x 8-32 B per wave instruction; from the tile each wave
            // stores a run of consecutive columns of one row (non-temporal:
            // the table is never re-read here)
            // the label part: a batch that goes to the redo launch (the condition of
            // the second attempt below, known once the walks are done) writes no row
            bool redo = false;
            if constexpr (P::label_part) {
                if (relAmb) atomicOr(&ctl->ambMask, 1u << l);
                fence_wg();
                __syncthreads();
                const bool tieBuf = tieDesc != nullptr &&
                                    __builtin_amdgcn_readfirstlane((int)(ld_wg(&tieDesc->req) != nullptr)) != 0;
                redo = !failed && (retry || (uni((int)ctl->ambMask) != 0 && !tieBuf));
            }
            if (!failed && !retry && !redo) {
                const int T = (int)tab.T;
                // (2 x NT entries of 21 B: inside the walk stacks' SMAX x NT x 8 B)
                double* const tLat = reinterpret_cast<double*>(smem + BCTRL_BYTES);
                double* const tRel = tLat + 2 * NT;
                int32_t* const tHop = reinterpret_cast<int32_t*>(tRel + 2 * NT);
                int32_t* const tPred = tHop + 2 * NT;
                uint8_t* const tFlg = reinterpret_cast<uint8_t*>(tPred + 2 * NT);
                const int wl = tid / NG, wc = tid % NG;     // writer: lane (row), column in block
                const int wrow = P::writes_rows ? laneRow[wl] : -1;
                const size_t wbase = (size_t)(wrow >= 0 ? wrow - tab.rowStart : 0) * (size_t)tab.T;
                __syncthreads();                            // walks done: stacks free
                // WQ targets per group per block, their loads issued branch-free
                // level by level (vertex id -> dist + label record + vertex
                // reliability -> parent vertex -> caller id), so WQ dependent
                // chains are in flight per thread and a block's two barriers are
                // shared by WQ x NG targets
                constexpr int WQ = 2;
                const int BW = WQ * NG;
                // the lane's own source (1-vertex igraph path [s]: the fold uses
                // edge (s,s), :1469-1488; the destination factor is skipped, :1457)
                const bool srcSelf = row >= 0 && g.hasSelf[src >= 0 ? src : 0];
                const double srcVrel = row >= 0 ? g.vrel[src >= 0 ? src : 0] : 1.0;
                const double selfL = srcSelf ? 0.0 + g.selfLat[src] : 0.0;
                const double selfR = srcSelf ? (1.0 * srcVrel) * g.selfRel[src] : 0.0;
                for (int j0 = 0; j0 < T; j0 += BW) {
                    int tq[WQ], pq[WQ];
                    unsigned long long dq[WQ];
                    Lbl rq[WQ];
                    double vq[WQ];
#pragma unroll
                    for (int q = 0; q < WQ; ++q) {
                        const int j = j0 + q * NG + gid;
                        tq[q] = row >= 0 && j < T ? g.attached[j] : -1;
                    }
#pragma unroll
                    for (int q = 0; q < WQ; ++q) {
                        const int tc = tq[q] >= 0 ? tq[q] : 0;
                        dq[q] = dec(ld_wg(&D[(size_t)tc * LB + l]));
                        rq[q] = lbl_ld(&LBL[(size_t)tc * LB + l]);
                        vq[q] = g.vrel[tc];
                    }
#pragma unroll
                    for (int q = 0; q < WQ; ++q) {
                        // (an unreachable target's record is not this batch's: its
                        // arc field is never followed)
                        const bool reach = tq[q] >= 0 && tq[q] != src && dq[q] != INF_BITS;
                        const int pa = reach ? rq[q].arc : -1;
                        const int x = g.inCol[pa >= 0 ? pa & ~TIE_AMB : 0];
                        pq[q] = pa >= 0 ? x : -1;
                    }
                    if (g.oldId) {
#pragma unroll
                        for (int q = 0; q < WQ; ++q) {
                            const int x = g.oldId[pq[q] >= 0 ? pq[q] : 0];   // device id -> caller's id
                            pq[q] = pq[q] >= 0 ? x : -1;
                        }
                    }
#pragma unroll
                    for (int q = 0; q < WQ; ++q) {
                        const int t = tq[q];
                        double L = 0.0, Rl = 0.0;
                        int h = -1, pv = -1;
                        uint8_t f = 0;
                        if (t >= 0) {
                            if (t == src) {
                                if (srcSelf) {
                                    L = selfL;
                                    Rl = selfR;
                                    h = 1;
                                } else {
                                    f |= F_NOEDGE;
                                }
                            } else if (dq[q] == INF_BITS) {
                                f |= F_UNREACHABLE;
                            } else {
                                L = b2d(dq[q]);
                                h = rq[q].hops;
                                pv = pq[q];
                                if (srcVrel == 1.0 && vq[q] == 1.0)
                                    Rl = rq[q].rel;
                                else
                                    Rl = fold_rel_batch<LB>(g.vrel, g.inRel, g.inCol, LBL, l, src, t, h);
                                if (L == 0.0) {                 // topology.c:1848-1852
                                    L = 1.0;
                                    f |= F_ZEROLAT;
                                }
                            }
                        }
                        const int ti = l * BW + q * NG + gid;
                        tLat[ti] = L;
                        tRel[ti] = Rl;
                        tHop[ti] = h;
                        tPred[ti] = pv;
                        tFlg[ti] = f;
                    }
                    __syncthreads();
#pragma unroll
                    for (int q = 0; q < WQ; ++q) {
                        const int c = j0 + q * NG + wc;
                        if (wrow >= 0 && c < T) {
                            const int ti2 = wl * BW + q * NG + wc;
                            const size_t o = wbase + (size_t)c;
                            __builtin_nontemporal_store(tLat[ti2], &tab.lat[o]);
                            __builtin_nontemporal_store(tRel[ti2], &tab.rel[o]);
                            __builtin_nontemporal_store(tHop[ti2], &tab.hops[o]);
                            __builtin_nontemporal_store(tFlg[ti2], &tab.flags[o]);
                            if (tab.pred) __builtin_nontemporal_store(tPred[ti2], &tab.pred[o]);
                        }
                    }
                    __syncthreads();
                }
            }
            if (relAmb) atomicOr(&ctl->ambMask, 1u << l);
            fence_wg();
            __syncthreads();
            // rows whose target paths meet an ambiguous entry (or that hit the
            // phase cap) go to k_exact_rows; their rows above are rewritten there
            needMask = failed ? LBMASK : ctl->ambMask;
            __syncthreads();
            if (tid == 0) ctl->ambMask = 0u;
            __syncthreads();
            // a tie row's export needs every vertex's parent: the full pass --
            // in line, or (the post kernel, with a deferred-export buffer) by
            // k_tie_export over the whole GPU after this kernel, so a tie batch
            // no longer runs a second full pass here (round 6: the c4q post
            // kernel was 43 vs 31 ms, a tie batch's in-line pass on its tail)
            const bool deferTie = P::defers_ties && tieDesc != nullptr &&
                                  __builtin_amdgcn_readfirstlane((int)(ld_wg(&tieDesc->req) != nullptr)) != 0;
            if constexpr (P::label_part) {
                if (redo && tid == 0) {      // -> PART 2 over bs.redo, after this kernel
                    int32_t* const rd = as_global(bs.redo);
                    rd[REDO_LIST + atomicAdd(&rd[0], 1)] = b;
                    atomicAdd(&rd[1], 1);
                }
                needMask = redo ? 0u : needMask;
                lastFull = false;
                break;
            }
            if (!fullPred && !failed && (retry || (needMask && !deferTie))) continue;
            lastFull = fullPred;
            break;
        }   // attempts
        if constexpr (P::exports_ties) {
            if (dbg && tid == 0) ctl->t3 = (long long)clock64();

            // ---- tie export: hand k_exact_rows the final distances, the parents
            // and the ambiguous entries, so it emulates the heap only until the
            // last tied predecessor is popped (tie threshold) ----
            if (needMask && !failed && tieDesc) {
                // descriptor read from memory here only: as a kernel argument
                // it cost the hot loops registers (SGPR spills)
                const TieBuf tie = *tieDesc;
                // deferred (attempt 0 of the post kernel): the slot records the
                // request, k_tie_export fills it after this kernel
                const bool defer = P::defers_ties && !lastFull;
                if (tid < LB) {
                    int sl = -1;
                    if ((needMask >> tid) & 1u) {
                        sl = atomicAdd(tie.count, 1);
                        if (sl >= tie.cap) sl = -1;
                    }
                    tieSlot[tid] = sl;
                    tieThr[tid] = 0ull;
                    if (defer && sl >= 0) {       // thread tid < LB is lane tid of group 0
                        tie.thr[sl] = 0.0;
                        tie.req[4 * sl + 0] = b;
                        tie.req[4 * sl + 1] = tid;
                        tie.req[4 * sl + 2] = src;
                        tie.req[4 * sl + 3] = *tie.round;
                    }
                }
                __syncthreads();
                const int sl = defer ? -1 : tieSlot[l];
                unsigned long long thr = 0ull;
                for (int v = gid; v < n; v += NG) {
                    if (sl < 0) continue;
                    const size_t e = (size_t)v * LB + l;
                    const int pe = lbl_arc(&LBL[e]);
                    const bool am = pe >= 0 && (pe & TIE_AMB);
                    const size_t o = (size_t)sl * (size_t)tie.n + v;
                    tie.D[o] = b2d(dec(ld_wg(&D[(size_t)v * LB + l])));
                    tie.P[o] = pe;
                    if (am) {   // rare: re-derive the tied (minimum tight) predecessor distance
                        const unsigned long long dv = dec(ld_wg(&D[(size_t)v * LB + l]));
                        const int a0 = undirected ? g.rowPtr[v] : g.inPtr[v];
                        const int a1 = undirected ? g.rowPtr[v + 1] : g.inPtr[v + 1];
                        unsigned long long mt = INF_BITS;
                        for (int a = a0; a < a1; ++a) {
                            const int u = undirected ? g.col[a] : g.inCol[a];
                            const double w = undirected ? g.lat[a] : g.inLat[a];
                            const unsigned long long du = dec(ld_wg(&D[(size_t)u * LB + l]));
                            if (du <= dv && d2b(b2d(du) + w) == dv && du < mt) mt = du;
                        }
                        if (mt != INF_BITS) thr = mt > thr ? mt : thr;
                    }
                }
                if (thr) atomicMax(&tieThr[l], thr);
                fence_wg();
                __syncthreads();
                if (!defer && gid == 0 && sl >= 0) tie.thr[sl] = b2d(tieThr[l]);
            } else if (tid < LB) {
                tieSlot[tid] = -1;
            }
            __syncthreads();
            if (dbg && tid == 0) ctl->t4 = (long long)clock64();
            // 0 fast path, 1 full igraph-heap emulation, 2 + slot: early-stop
            // emulation with the exported tie data
            if (gid == 0 && row >= 0)
                rowAmbig[(size_t)b * LB + l] =
                    ((needMask >> l) & 1u) ? (uint8_t)(tieSlot[l] >= 0 ? 2 + tieSlot[l] : 1) : (uint8_t)0;
        }
        // ---- debug epilogue, the one of every part (SHD_PE_DEBUG_COUNTERS): the batch's
        // slots dbg[16 b + k] and the parts that own them.  Stored: 0 phases, 15 repairs, 5 relax kcycles (t1 - t0): PART 0, 1;
        // 6 predecessor pass (t2 - t1): 0, 2, 4, 5; 2 label walks (after the walks),
        // 3 needMask, 7 labels + rows (t3 - t2), 11 tie export (t4 - t3), 8 after it:
        // 0, 2, 4, 6; 1 the SHDPE_DIAG_WHY word: 0, 2, 4.  Added (atomicAdd / atomicOr
        // onto what another kernel or phase of the round left): 4 vertex processings,
        // 9 arcs / 16, 10 active lanes, and in the relax 12, 13, 14 busy max, busy
        // mean, queue entries per phase: 0, 1; 1 the DIAG word: 5, 6; predCnt (the
        // on-demand pass's in-arcs claimed, gathered): 0, 2, 4, 5, not the redo launch,
        // whose batches the predecessor part counted.
        if constexpr (!P::exports_ties) __syncthreads();     // (the tie export ends on a barrier)
#ifdef SHDPE_DIAG_WHY
        if (P::exports_ties && failed) why |= 1u;
        if (why) atomicOr(&ctl->dWhy, why);
        __syncthreads();
#endif
        if (dbg && tid == 0) {
            if constexpr (P::relaxes) {
                dbg[16 * b + 0] = phases;
                dbg[16 * b + 5] = (int)((ctl->t1 - ctl->t0) >> 10);
                dbg[16 * b + 15] = repairs;
                atomicAdd(&dbg[16 * b + 4], (int)ctl->dProcs);
                atomicAdd(&dbg[16 * b + 9], (int)(ctl->dArcs >> 4));
                atomicAdd(&dbg[16 * b + 10], (int)ctl->dLanes);
            }
            if constexpr (!P::relax_part) {
                if (P::has_labels_in_bs) atomicOr(&dbg[16 * b + 1], (int)ctl->dWhy);
                else dbg[16 * b + 1] = (int)ctl->dWhy;
            }
            if constexpr (P::exports_ties) dbg[16 * b + 3] = (int)needMask;
            if constexpr (P::runs_pred_pass) dbg[16 * b + 6] = (int)((ctl->t2 - ctl->t1) >> 10);
            if constexpr (P::exports_ties) {
                dbg[16 * b + 7] = (int)((ctl->t3 - ctl->t2) >> 10);
                dbg[16 * b + 11] = (int)((ctl->t4 - ctl->t3) >> 10);
            }
            if constexpr (P::runs_pred_pass)
                if (bs.predCnt && !(PART == 2 && bs.redoRun)) {
                    atomicAdd(as_global(bs.predCnt), (unsigned long long)ctl->dClaim);
                    atomicAdd(as_global(bs.predCnt) + 1, (unsigned long long)ctl->dGath);
                }
        }
        if constexpr (P::exports_ties) fence_wg();
        __syncthreads();
        if constexpr (P::exports_ties)
            if (dbg && tid == 0) dbg[16 * b + 8] = (int)(((long long)clock64() - ctl->t4) >> 10);
    }
}

// The igraph parent of a vertex at distance dv, from a batch's persisted
// distance array D ([vertex][LB], lane l), over the vertex's in-arcs [a0, a1)
// (its own row when undirected): the first tight in-arc, in incidence order,
// of minimum dist[u].  The one statement of the rule for k_tie_export and
// k_tree_load.  best: that minimum (INF_BITS: no tight arc); cnt: tight arcs
// that attain it; arc: the first of them; mn: the least dist[u] + w over every
// in-arc (mn < dv: a Bellman violation).
struct ParentPick {
    unsigned long long best, mn;
    int cnt, arc;
    // equal minima, a zero-increment arc (or no tight arc at all): the heap decides
    __device__ __forceinline__ bool ambiguous(unsigned long long dv) const { return cnt != 1 || best == dv; }
};
__device__ __forceinline__ ParentPick pick_parent(const DevGraph& g, bool undirected,
                                                  const unsigned long long* __restrict__ D, int LB, int l, int a0,
                                                  int a1, unsigned long long dv) {
    ParentPick k{INF_BITS, INF_BITS, 0, -1};
    for (int a = a0; a < a1; ++a) {
        const int u = undirected ? g.col[a] : g.inCol[a];
        const double w = undirected ? g.lat[a] : g.inLat[a];
        const unsigned long long du = dec(D[(size_t)u * LB + l]);
        const double cand = b2d(du) + w;
        const unsigned long long cb = d2b(cand);
        k.mn = cb < k.mn ? cb : k.mn;
        if (dv != INF_BITS && du <= dv && cand == b2d(dv)) {
            if (du < k.best) {
                k.best = du;
                k.cnt = 1;
                k.arc = a;
            } else if (du == k.best) {
                ++k.cnt;
            }
        }
    }
    return k;
}

// k_tie_export: the deferred tie export of one round (launch_tie_export).
// One thread per (slot, vertex), grid-stride: the vertex's distance, and its
// parent exactly as the post kernel's full predecessor pass derives it (first
// in-arc, in incidence order, among the tight ones with minimum dist[u];
// TIE_AMB on equal minima or a zero-increment arc; -1 for the source and
// unreachable vertices), the threshold as the maximum tied-predecessor
// distance over the ambiguous entries (k_exact_rows' early stop), and the
// Bellman check over every in-arc (a violation sends the row to the full
// emulation, rowAmbig 1, as a failed batch would).  violSlot >= 0 (tests,
// SHDPE_TIE_CORRUPT=3): that slot's row is treated as violated.
template <int LB>
__global__ __launch_bounds__(256) void k_tie_export(DevGraph g0, BatchScratch bs, TieBuf tie, int round,
                                                    uint8_t* __restrict__ rowAmbig, int violSlot) {
    const DevGraph g = global_view(g0);
    const int n = g.n;
    const bool undirected = g.inCol == g.col;
    const int cnt = min(*as_global(tie.count), tie.cap);
    const size_t SE = (size_t)bs.nStride * LB;
    const size_t total = (size_t)cnt * (size_t)n;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int sl = (int)(i / (size_t)n);
        const int v = (int)(i % (size_t)n);
        const int32_t* rq = as_global(tie.req) + 4 * sl;
        if (rq[3] != round) continue;
        const int b = rq[0], l = rq[1], src = rq[2];
        const unsigned long long* D = as_global(bs.D) + (size_t)b * SE;
        const unsigned long long dv = dec(D[(size_t)v * LB + l]);
        const size_t o = (size_t)sl * (size_t)tie.n + v;
        as_global(tie.D)[o] = b2d(dv);
        int pe = -1;
        if (v != src) {
            const int a0 = undirected ? g.rowPtr[v] : g.inPtr[v];
            const int a1 = undirected ? g.rowPtr[v + 1] : g.inPtr[v + 1];
            const ParentPick k = pick_parent(g, undirected, D, LB, l, a0, a1, dv);
            if (k.mn < dv || sl == violSlot) rowAmbig[(size_t)b * LB + l] = 1;   // Bellman violation: full emulation
            if (dv != INF_BITS) {
                const bool ea = k.ambiguous(dv);
                pe = ea ? (TIE_AMB | (k.arc > 0 ? k.arc : 0)) : k.arc;
                if (ea && k.best != INF_BITS)
                    atomicMax(reinterpret_cast<unsigned long long*>(as_global(tie.thr) + sl), k.best);
            }
        }
        as_global(tie.P)[o] = pe;
    }
}

void launch_tie_export(const DevGraph& g, const BatchScratch& bs, int lb, const TieBuf& tie, int round,
                       uint8_t* dRowAmbig, int grid, int violSlot, void* stream) {
    if (tie.cap <= 0 || !tie.req) return;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (lb == 4)
        hipLaunchKernelGGL(k_tie_export<4>, dim3(grid), dim3(256), 0, st, g, bs, tie, round, dRowAmbig, violSlot);
    else if (lb == 8)
        hipLaunchKernelGGL(k_tie_export<8>, dim3(grid), dim3(256), 0, st, g, bs, tie, round, dRowAmbig, violSlot);
    else if (lb == 32)
        hipLaunchKernelGGL(k_tie_export<32>, dim3(grid), dim3(256), 0, st, g, bs, tie, round, dRowAmbig, violSlot);
    else
        hipLaunchKernelGGL(k_tie_export<16>, dim3(grid), dim3(256), 0, st, g, bs, tie, round, dRowAmbig, violSlot);
}

// k_paths_walk_dist (shd_pe_get_paths, launch_paths_walk_dist): the paths of
// requests whose source sits in a round of the split kernels, walked over the
// round's persisted distance arrays after its post kernel (the labels L are
// per workgroup and reused by the workgroup's next batch; the distances are
// per batch).  One thread per request, len - 1 steps from the destination: at
// each vertex the parent exactly as the post kernel's predecessor pass and
// k_tie_export derive it -- the tight in-arc with minimum dist[u] -- and
// nothing else: equal minima, a zero-increment arc, a Bellman violation at the
// vertex, a lane the post kernel flagged (rowAmbig: a tie row, a failed batch)
// or a walk that does not end on the source at distance 0 hands the request on
// (failed[req] = 1; the grouped emulation serves it).
__global__ __launch_bounds__(256) void k_paths_walk_dist(DevGraph g0, BatchScratch bs, PathsDistArgs p) {
    const DevGraph g = global_view(g0);
    const int32_t j = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (j >= p.nReqs) return;
    const PathReq q = as_global(p.reqs)[j];
    const int32_t L = as_global(p.len)[q.req];
    if (L <= 0) return;
    uint8_t* failed = as_global(p.failed);
    const int slot = q.slot - p.slotBase;
    if (as_global(p.rowAmbig)[slot] != 0) { failed[q.req] = 1; return; }
    const int LB = p.lb;
    const int b = slot / LB, l = slot % LB;
    const unsigned long long* __restrict__ D = as_global(bs.D) + (size_t)b * ((size_t)bs.nStride * LB);
    int32_t* __restrict__ out = as_global(p.verts) + as_global(p.off)[q.req];
    const bool undirected = g.inCol == g.col;
    int v = q.t;
    unsigned long long dv = dec(D[(size_t)v * LB + l]);
    bool ok = dv != INF_BITS;
    for (int32_t k = L - 1; k >= 1 && ok; --k) {
        out[k] = g.oldId ? g.oldId[v] : v;
        const int a0 = undirected ? g.rowPtr[v] : g.inPtr[v];
        const int a1 = undirected ? g.rowPtr[v + 1] : g.inPtr[v + 1];
        unsigned long long best = INF_BITS, mn = INF_BITS;
        int cnt = 0, bu = -1;
        for (int a = a0; a < a1; ++a) {
            const int u = undirected ? g.col[a] : g.inCol[a];
            const double w = undirected ? g.lat[a] : g.inLat[a];
            const unsigned long long du = dec(D[(size_t)u * LB + l]);
            const double cand = b2d(du) + w;
            const unsigned long long cb = d2b(cand);
            mn = cb < mn ? cb : mn;
            if (du <= dv && cand == b2d(dv)) {
                if (du < best) { best = du; cnt = 1; bu = u; }
                else if (du == best) ++cnt;
            }
        }
        if (mn < dv || cnt != 1 || best == dv) { ok = false; break; }
        v = bu;
        dv = best;
    }
    if (ok && v == q.s && dv == 0ull) out[0] = g.oldId ? g.oldId[v] : v;
    else failed[q.req] = 1;
}

void launch_paths_walk_dist(const DevGraph& g, const BatchScratch& bs, const PathsDistArgs& a, void* stream) {
    if (a.nReqs <= 0) return;
    hipLaunchKernelGGL(k_paths_walk_dist, dim3((unsigned)((a.nReqs + 255) / 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), g, bs, a);
}

// k_tree_load (shd_pe_table_load, launch_tree_load): the all-pairs load of the
// sources of one round of the split kernels, from the round's persisted
// distance arrays after its post kernel and tie export.  The shortest paths of
// a source form a tree, the load of a vertex is the weight seeded in its
// subtree and the load of its parent arc is the same number, so every parent is
// derived once per (source, vertex) and one leaves-first sum replaces T walks.
//
// Persistent workgroups, one batch at a time, each with a private scratch slot
// of (parent, sum, pending children) per (vertex, lane) that it reuses for its
// next batch.  Per batch, with a workgroup barrier between the steps:
//   init    the slot: unclaimed, 0, 0; per lane whether it runs at all (a pad,
//           a lane the pass flagged: not started)
//   seed    per (destination, lane): status and hops from the table row ->
//           the lane's totals and expected sum; a status-0 destination of
//           non-zero weight adds its weight to its vertex and
//   claim   walks up from it until it meets a claimed vertex: each vertex it
//           claims derives its parent (pick_parent) and counts itself as that
//           parent's child.  Equal minima, a zero-increment arc, a Bellman
//           violation, an infinite distance or hops the table cannot hold fail
//           the lane
//   sum     a scan offers every claimed entry with no pending child; who takes
//           an entry (compare-and-swap 0 -> TREE_TAKEN on its pending count)
//           adds its sum to the parent's, counts down the parent's pending
//           children and, on the last, offers the parent in the same way
//   check   a lane passes when it did not fail and its source's sum is the
//           expected one; any other started lane is handed on (handed = 1)
//   commit  one thread per vertex: the passing lanes' sums, those that share
//           the parent combined first, added to the vertex's place in acc and
//           to the place of the arc from the parent (caller's ids, find_arc as
//           k_paths_load finds it) with device-scope no-return 64-bit adds.
//           Within a batch the places of different vertices differ, so this
//           combining is all there is to combine.
// Nothing reaches acc or the totals before the lane's check.  The slot's
// atomics are workgroup traffic (workgroup scope); the sums are integers mod
// 2^64, so every order gives the same result.
constexpr int TREE_THREADS = 512;
constexpr int32_t TREE_FREE = -1, TREE_SOURCE = -2, TREE_BUSY = -3;   // parent words that are no in-arc
constexpr int32_t TREE_TAKEN = -1;                                    // pending word of a summed entry

__device__ __forceinline__ void tree_add(unsigned long long* p, unsigned long long v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__global__ __launch_bounds__(TREE_THREADS) void k_tree_load(DevGraph g0, DevGraph aux0, DevTable tab0,
                                                            BatchScratch bs, TreeLoadArgs p) {
    __shared__ unsigned long long expect[32], tot[32][3], issuedWg, claimedWg;
    __shared__ unsigned int bad[32];             // requests with a status
    __shared__ int srcOf[32], posOf[32], run[32], fail[32], pass[32];
    const DevGraph g = global_view(g0);
    const DevGraph aux = global_view(aux0);
    const DevTable tab = global_view(tab0);
    const int tid = threadIdx.x, n = g.n, LB = p.lb;
    const int64_t T = tab.T;
    const bool undirected = g.inCol == g.col;
    const size_t SE = (size_t)bs.nStride * LB, NE = (size_t)n * LB;
    int32_t* __restrict__ par = as_global(p.par) + (size_t)blockIdx.x * NE;
    unsigned long long* __restrict__ sum = (unsigned long long*)as_global(p.sum) + (size_t)blockIdx.x * NE;
    int32_t* __restrict__ pend = as_global(p.pend) + (size_t)blockIdx.x * NE;
    const int32_t* __restrict__ attDev = as_global(p.attDev);
    unsigned long long* __restrict__ acc = (unsigned long long*)as_global(p.acc);
    unsigned long long* __restrict__ out = (unsigned long long*)as_global(p.out);
    if (tid == 0) issuedWg = claimedWg = 0;
    for (int b = blockIdx.x; b < p.nBatches; b += gridDim.x) {
        const unsigned long long* __restrict__ D = as_global(bs.D) + (size_t)b * SE;
        const unsigned long long* __restrict__ W =
            p.weight ? (const unsigned long long*)as_global(p.weight) + (size_t)b * LB * (size_t)T : nullptr;
        // ---- init
        if (tid < LB) {
            const int pos = as_global(p.batchRows)[b * LB + tid];
            posOf[tid] = pos;
            run[tid] = pos >= 0 && as_global(p.rowAmbig)[b * LB + tid] == 0;
            srcOf[tid] = pos >= 0 ? attDev[pos] : -1;
            fail[tid] = pass[tid] = 0;
            expect[tid] = tot[tid][0] = tot[tid][1] = tot[tid][2] = 0;
            bad[tid] = 0;
        }
        for (size_t i = tid; i < NE; i += TREE_THREADS) {
            par[i] = TREE_FREE;
            sum[i] = 0;
            pend[i] = 0;
        }
        fence_wg();
        __syncthreads();
        // ---- seed and claim
        for (size_t i = tid; i < (size_t)T * LB; i += TREE_THREADS) {
            const int q = (int)(i / LB), l = (int)(i % LB);
            if (!run[l]) continue;
            const int pos = posOf[l], src = srcOf[l];
            unsigned long long hops = 0;
            if (q != pos) {
                const size_t cell = (size_t)(pos - tab.rowStart) * (size_t)T + (size_t)q;
                if (tab.flags[cell] & (F_UNREACHABLE | F_NOEDGE)) {
                    atomicAdd(&bad[l], 1u);
                    continue;
                }
                const int h = tab.hops[cell];
                if (h < 1 || h >= n) {           // (not a table this engine wrote: the request route says so)
                    fail[l] = 1;
                    continue;
                }
                hops = (unsigned long long)h;
            }
            const unsigned long long w = W ? W[(size_t)l * (size_t)T + q] : 1ull;
            atomicAdd(&tot[l][0], 1ull);
            if (w == 0) continue;                // adds nothing anywhere
            atomicAdd(&tot[l][1], w * (hops + 1));
            atomicAdd(&tot[l][2], w * hops);
            atomicAdd(&expect[l], w);
            int x = attDev[q];
            tree_add(&sum[(size_t)x * LB + l], w);
            const bool spoil = p.corrupt == 2 && b * LB + l == p.corruptSlot;
            while (!*(volatile int*)&fail[l]) {
                const size_t e = (size_t)x * LB + l;
                int32_t was = TREE_FREE;
                if (!__hip_atomic_compare_exchange_strong(&par[e], &was, TREE_BUSY, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                          __HIP_MEMORY_SCOPE_WORKGROUP))
                    break;                       // claimed already: the rest of the way is too
                const unsigned long long dv = dec(D[e]);
                if (x == src) {
                    if (dv != 0ull) fail[l] = 1;
                    __hip_atomic_store(&par[e], TREE_SOURCE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    break;
                }
                const int a0 = undirected ? g.rowPtr[x] : g.inPtr[x];
                const int a1 = undirected ? g.rowPtr[x + 1] : g.inPtr[x + 1];
                const ParentPick k = pick_parent(g, undirected, D, LB, l, a0, a1, dv);
                if (dv == INF_BITS || k.mn < dv || k.ambiguous(dv) || spoil) {
                    fail[l] = 1;
                    break;
                }
                const int u = g.inCol[k.arc];    // (undirected: inCol is col)
                __hip_atomic_store(&par[e], k.arc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_add(&pend[(size_t)u * LB + l], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                x = u;                           // (dist[u] < dist[x]: the walk ends)
            }
        }
        fence_wg();
        __syncthreads();
        // ---- sum, leaves first
        for (size_t i = tid; i < NE; i += TREE_THREADS) {
            const int l = (int)(i % LB);
            if (!run[l] || fail[l]) continue;
            const int32_t pa0 = ld_wg(&par[i]);
            if (pa0 == TREE_FREE || pa0 == TREE_BUSY) continue;
            size_t e = i;
            for (;;) {
                int32_t zero = 0;
                if (!__hip_atomic_compare_exchange_strong(&pend[e], &zero, TREE_TAKEN, __ATOMIC_ACQUIRE,
                                                          __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
                    break;                       // children pending, or taken by another thread
                const int32_t pa = ld_wg(&par[e]);
                if (pa < 0) break;               // the source: its sum stays for the check
                // (the entry's sum is final: every child added before it counted down)
                const unsigned long long s = __hip_atomic_fetch_add(&sum[e], 0ull, __ATOMIC_RELAXED,
                                                                    __HIP_MEMORY_SCOPE_WORKGROUP);
                const size_t eu = (size_t)g.inCol[pa] * LB + l;
                tree_add(&sum[eu], s);
                if (__hip_atomic_fetch_sub(&pend[eu], 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP) != 1) break;
                e = eu;
            }
        }
        fence_wg();
        __syncthreads();
        // ---- check
        if (tid < LB && run[tid]) {
            const int l = tid;
            unsigned long long want = expect[l];
            if (p.corrupt == 1 && b * LB + l == p.corruptSlot) want += 1;
            const unsigned long long got = __hip_atomic_fetch_add(&sum[(size_t)srcOf[l] * LB + l], 0ull, __ATOMIC_RELAXED,
                                                                  __HIP_MEMORY_SCOPE_WORKGROUP);
            const bool ok = !fail[l] && got == want;
            pass[l] = ok;
            as_global(p.handed)[b * LB + l] = ok ? 0 : 1;
            if (ok) {
                __hip_atomic_fetch_add(&out[0], tot[l][0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_add(&out[1], tot[l][1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_add(&out[2], tot[l][2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_add(&out[3], (unsigned long long)bad[l], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_add(&out[4], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        __syncthreads();
        // ---- commit
        unsigned long long issued = 0, claimed = 0;
        for (int v = tid; v < n; v += TREE_THREADS) {
            const size_t e0 = (size_t)v * LB;
            unsigned long long vsum = 0;
            unsigned int todo = 0;               // passing lanes with a parent arc, not yet combined
            for (int l = 0; l < LB; ++l) {
                if (!pass[l]) continue;
                const int32_t pa = ld_wg(&par[e0 + l]);
                if (pa == TREE_FREE || pa == TREE_BUSY) continue;
                ++claimed;
                vsum += ld_wg(&sum[e0 + l]);
                if (pa >= 0) todo |= 1u << l;
            }
            if (todo == 0 && vsum == 0) continue;
            const int ov = g.oldId ? g.oldId[v] : v;
            if (vsum) {
                __hip_atomic_fetch_add(acc + p.nArcs + ov, vsum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                ++issued;
            }
            while (todo) {
                const int l = __ffs(todo) - 1;
                const int32_t pa = ld_wg(&par[e0 + l]);
                unsigned long long asum = 0;
                for (int m = l; m < LB; ++m)
                    if (((todo >> m) & 1u) && ld_wg(&par[e0 + m]) == pa) {
                        asum += ld_wg(&sum[e0 + m]);
                        todo &= ~(1u << m);
                    }
                if (asum == 0) continue;
                const int u = g.inCol[pa];
                const int ou = g.oldId ? g.oldId[u] : u;
                int a = -1;
                if (ou != ov && find_arc(aux, ou, ov, &a)) {
                    __hip_atomic_fetch_add(acc + a, asum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    ++issued;
                } else {                         // (never: a parent arc is an arc of the graph)
                    __hip_atomic_fetch_add(&out[7], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
        if (claimed) atomicAdd(&claimedWg, claimed);
        if (issued) atomicAdd(&issuedWg, issued);
        __syncthreads();                         // the slot is free for the next batch
    }
    if (tid == 0) {
        if (claimedWg) __hip_atomic_fetch_add(&out[5], claimedWg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (issuedWg) __hip_atomic_fetch_add(&out[6], issuedWg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

void launch_tree_load(const DevGraph& g, const DevGraph& gAux, const DevTable& tab, const BatchScratch& bs,
                      const TreeLoadArgs& a, int grid, void* stream) {
    if (a.nBatches <= 0 || grid <= 0) return;
    hipLaunchKernelGGL(k_tree_load, dim3((unsigned)(grid < a.nBatches ? grid : a.nBatches)), dim3(TREE_THREADS), 0,
                       reinterpret_cast<hipStream_t>(stream), g, gAux, tab, bs, a);
}

int batch_threads(int wpe) { return wpe == 6 ? 768 : BT_THREADS; }

// LDS of a variant's part.  The predecessor part (5) holds the pending and
// claim bitmaps and its heavy list, the label part (6) the walk stacks (the
// writer's tile lies inside them); the whole-batch kernel and the unsplit post
// kernel (0, 2, 4) reuse the bitmaps' room for the stacks, so they take the
// larger of the two, and the relax (1) keeps that size: its in-arc flag bits
// live behind the bitmaps in it (batch_relax_flags).
int batch_lds_bytes(int n, int wpe, bool gbits, int part) {
    const int nwp = (((n + 31) >> 5) + 3) & ~3;
    const int stack = batch_threads(wpe) * (wpe >= 6 ? BCfg<8>::SMAX : BCfg<4>::SMAX) * 8;
    const int bits = gbits ? 0 : 2 * 4 * nwp;
    if (part == 5) return BCTRL_BYTES + bits + 4 * pred_heavy_cap(nwp, gbits);
    if (part == 6) return BCTRL_BYTES + stack;
    return BCTRL_BYTES + (bits > stack ? bits : stack);
}

int64_t batch_bits_words(int n) { return 2 * (int64_t)((((n + 31) >> 5) + 3) & ~3); }

// predecessor filter: the plain relax of this variant flags in-arcs when a
// batch's bits fit in its LDS behind the pending bitmaps (C4: 75 KB in the
// 4-wave variant's 128 KB, not in the 6- and 8-wave variants' 49 / 64 KB);
// behind any other relax the post kernel reads every in-arc
bool batch_relax_flags(const BatchScratch& bs, const BatchLaunch& cfg, int n) {
    return bs.arcHit && !cfg.gbits && cfg.split &&
           (int64_t)BCTRL_BYTES + 4 * batch_bits_words(n) + bs.mStride / 8 <= (int64_t)cfg.ldsBytes;
}

// Every instantiation of k_batch_rows, by (lb, wpe, gbits, part): LB 4 / 8 /
// 16 / 32 with LDS bitmaps and LB 16 with global ones (graphs whose bitmaps
// exceed LDS: the engine forces LB 16), at 4 / 6 / 8 waves, PART 0 / 1 / 2 / 4 /
// 5, and PART 6 (no bitmaps: one instantiation serves both).
using BatchKernel = void (*)(DevGraph, DevTable, BatchScratch, const int32_t*, int32_t, uint8_t*, double,
                             int32_t*, const TieBuf*);
struct BatchVariant {
    int lb, wpe;
    bool gbits;
    int part;
    BatchKernel fn;
};
#define BATCH_PARTS(LB, WPE, GB)                                                              \
    {LB, WPE, GB, 0, &k_batch_rows<LB, WPE, GB, 0>}, {LB, WPE, GB, 1, &k_batch_rows<LB, WPE, GB, 1>}, \
    {LB, WPE, GB, 2, &k_batch_rows<LB, WPE, GB, 2>}, {LB, WPE, GB, 4, &k_batch_rows<LB, WPE, GB, 4>}, \
    {LB, WPE, GB, 5, &k_batch_rows<LB, WPE, GB, 5>}
#define BATCH_LABEL(LB, WPE) {LB, WPE, false, 6, &k_batch_rows<LB, WPE, false, 6>}
#define BATCH_WIDTHS(WPE)                                                                     \
    BATCH_PARTS(4, WPE, false), BATCH_PARTS(8, WPE, false), BATCH_PARTS(16, WPE, false),      \
    BATCH_PARTS(32, WPE, false), BATCH_PARTS(16, WPE, true), BATCH_LABEL(4, WPE),             \
    BATCH_LABEL(8, WPE), BATCH_LABEL(16, WPE), BATCH_LABEL(32, WPE)
static const BatchVariant BATCH_VARIANTS[] = {BATCH_WIDTHS(4), BATCH_WIDTHS(6), BATCH_WIDTHS(8)};
#undef BATCH_WIDTHS
#undef BATCH_LABEL
#undef BATCH_PARTS

// the variant that serves a request: any other width runs LB 16, any other
// wave count 4 (8 and above: 8), any other part the whole-batch kernel
static BatchKernel batch_kernel(int lb, int wpe, bool gbits, int part) {
    lb = gbits || (lb != 4 && lb != 8 && lb != 32) ? 16 : lb;
    wpe = wpe >= 8 ? 8 : wpe == 6 ? 6 : 4;
    part = part == 1 || part == 2 || part == 4 || part == 5 || part == 6 ? part : 0;
    if (part == 6) gbits = false;
    for (const BatchVariant& v : BATCH_VARIANTS)
        if (v.lb == lb && v.wpe == wpe && v.gbits == gbits && v.part == part) return v.fn;
    return nullptr;     // not reached: the table holds every normalised key
}

const void* batch_kernel_ptr(int lb, int wpe, bool gbits, int part) {
    return reinterpret_cast<const void*>(batch_kernel(lb, wpe, gbits, part));
}

void launch_batch_rows(const DevGraph& g, const DevTable& tab, const BatchScratch& bs,
                       const int32_t* dBatchRows, int32_t nBatches, uint8_t* dRowAmbig,
                       const BatchLaunch& cfg, int32_t* dDbg, const TieBuf* tie, void* stream, int part) {
    if (nBatches <= 0) return;
    const int grid = nBatches < cfg.grid ? nBatches : cfg.grid;
    if (grid <= 0) return;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    BatchScratch bsl = bs;
    bsl.hitLds = part == 1 && batch_relax_flags(bs, cfg, g.n);
    // (the redo launch: PART 2 over the list the label part left, bs.redoRun set by the caller)
    bsl.redoRun = part == 2 && bs.redoRun && bs.redo ? 1 : 0;
    const BatchKernel fn = batch_kernel(cfg.lb, cfg.wpe, cfg.gbits != 0, part);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                              cfg.ldsBytes);
    // (the kernel's NT is compile-time: the variant's own size, batch_threads)
    hipLaunchKernelGGL(fn, dim3(grid), dim3(batch_threads(cfg.wpe)), cfg.ldsBytes, st, g, tab, bsl, dBatchRows,
                       nBatches, dRowAmbig, cfg.delta, dDbg, tie);
}

}  // namespace shdpe
