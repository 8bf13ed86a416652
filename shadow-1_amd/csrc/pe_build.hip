// pe_build.hip -- the engine's graph built on the device.
//
// shd_pe_create_built(SHD_PE_BUILD_DEVICE) goes from the caller's edge list to
// the arrays of DevGraph without a host CSR: what build_host_graph
// (pe_graph.cpp) and upload_graph (pe_engine.hip) make for the same
// description, byte for byte, HostGraph read back from the device.  The rules
// are build_host_graph's (cited there to topology.c); the construction:
//
//   k_build_vertex   vertex packetloss range, vrel = 1 - loss (NaN: absent)
//   k_build_count    validates every edge; per row the arc count (one atomic
//                    per run of equal `from` in a wave: GraphML lists a
//                    complete graph's edges grouped by source); per vertex
//                    the loop count, the newest loop's edge id (atomicMax) and
//                    the minimum loop latency (atomicMin on its bit pattern)
//   k_build_selfmin  the newest loop among those of minimum latency
//   k_build_scan     exclusive scan of the counts -> rowPtr (inPtr); one
//                    workgroup, 64-bit sums: 2^31 - 1 arcs or more is an error
//   k_build_scatter  (neighbour, edge id) into the row's range at an atomic
//                    cursor: any order
//   k_build_rows     one workgroup per row: the neighbours set in an n-bit
//                    bitmap in LDS (a bit found set is a parallel edge), a
//                    prefix popcount per word, rank = prefix + popcount of the
//                    bits below; the arc is written at rowPtr[u] + rank and
//                    its position noted per (edge, side).  Directed graphs run
//                    it a second time over the in-arcs: the IN CSR by source id
//   k_build_link     per edge: the two noted positions are each other's
//                    outToIn (directed: the out-arc's is the in-arc's position)
//   k_build_vfinal   self-loop fields, completeness, multigraph edge counts
//
// Nothing depends on scheduling: the counts and the bitmap are sets, the rank
// is a function of the set, and every atomic maximum / minimum is unique.
// Ordering is kernel boundaries on one stream.  All stores are vector stores
// from plain C++.
//
// Two cases are handed to the host form: parallel edges (the merge and latFold
// rules stay there) and more vertices than the bitmap holds (BUILD_MAX_N).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cstring>

#include "pe_build.hpp"
#include "pe_stage.hpp"

namespace shdpe {

enum { BW_ERR = 0, BW_MULTI, BW_TOOBIG, BW_INCOMPLETE, BW_MAXSELF, BW_ANYSELF, BW_COUNT = 16 };

constexpr int BUILD_BLOCK = 256;
constexpr int BUILD_MAX_GRID = 4096;
constexpr int BUILD_SCAN_BLOCK = 1024;

__device__ __forceinline__ int build_lane() { return (int)(threadIdx.x & 63); }

__device__ __forceinline__ void build_flag(bool on, int32_t* word) {
    const unsigned long long b = __ballot(on);
    if (b != 0ull && build_lane() == (int)__ffsll((long long)b) - 1) *word = 1;
}

__device__ __forceinline__ bool edge_valid(int32_t f, int32_t t, double L, double p, int32_t n) {
    return (uint32_t)f < (uint32_t)n && (uint32_t)t < (uint32_t)n && L > 0.0 && p >= 0.0 && p <= 1.0;
}

// The run of equal keys this lane sits in (all 64 lanes call): the lane of
// the run's first element and, for that lane, the run's length.
__device__ __forceinline__ void wave_run(int32_t key, int& headLane, int& runLen) {
    const int lane = build_lane();
    const int32_t prev = __shfl_up(key, 1, 64);
    const bool head = lane == 0 || key != prev;
    const unsigned long long hb = __ballot(head);
    const unsigned long long upTo = (2ull << lane) - 1ull;              // lanes 0..lane (lane 63: all)
    headLane = 63 - __clzll((long long)(hb & upTo));
    const unsigned long long above = hb & ~upTo;
    runLen = (above ? (int)__ffsll((long long)above) - 1 : 64) - lane;
}

__global__ __launch_bounds__(BUILD_BLOCK) void k_build_vertex(const double* __restrict__ vloss, int32_t n,
                                                              double* __restrict__ vrel, int32_t* __restrict__ W) {
    const int32_t v = (int32_t)(blockIdx.x * BUILD_BLOCK + threadIdx.x);
    bool bad = false;
    if (v < n) {
        double r = 1.0;
        if (vloss) {
            const double p = vloss[v];
            if (!(p != p)) {
                bad = !(p >= 0.0 && p <= 1.0);
                r = 1.0 - p;
            }
        }
        vrel[v] = r;
    }
    build_flag(bad, &W[BW_ERR]);
}

__global__ __launch_bounds__(BUILD_BLOCK) void k_build_count(
    const int32_t* __restrict__ from, const int32_t* __restrict__ to, const double* __restrict__ lat,
    const double* __restrict__ loss, int64_t m, int32_t n, int32_t directed, int32_t* __restrict__ cnt,
    int32_t* __restrict__ cntIn, int32_t* __restrict__ nSelf, int32_t* __restrict__ selfNewest,
    unsigned long long* __restrict__ selfMinBits, int32_t* __restrict__ W) {
    const int lane = build_lane();
    const int64_t wave = (int64_t)blockIdx.x * (BUILD_BLOCK / 64) + (threadIdx.x >> 6);
    const int64_t step = (int64_t)gridDim.x * BUILD_BLOCK;
    bool bad = false, loop = false;
    for (int64_t base = wave * 64; base < m; base += step) {           // uniform per wave
        const int64_t e = base + lane;
        const bool in = e < m;
        const int32_t f = in ? from[e] : -1, t = in ? to[e] : -1;
        const double L = in ? lat[e] : 1.0, p = in ? loss[e] : 0.0;
        const bool ok = in && edge_valid(f, t, L, p, n);
        bad = bad || (in && !ok);
        const bool arc = ok && f != t;
        int headLane, runLen;
        wave_run(arc ? f : -1, headLane, runLen);
        if (arc && headLane == lane) atomicAdd(&cnt[f], runLen);
        if (arc) atomicAdd(directed ? &cntIn[t] : &cnt[t], 1);
        if (ok && f == t) {
            loop = true;
            atomicAdd(&nSelf[f], 1);
            atomicMax(&selfNewest[f], (int32_t)e);
            atomicMin(&selfMinBits[f], (unsigned long long)__double_as_longlong(L));
        }
    }
    build_flag(bad, &W[BW_ERR]);
    build_flag(loop, &W[BW_ANYSELF]);
}

__global__ __launch_bounds__(BUILD_BLOCK) void k_build_selfmin(const int32_t* __restrict__ from,
                                                               const int32_t* __restrict__ to,
                                                               const double* __restrict__ lat, int64_t m, int32_t n,
                                                               const unsigned long long* __restrict__ selfMinBits,
                                                               int32_t* __restrict__ selfMinId) {
    const int64_t step = (int64_t)gridDim.x * BUILD_BLOCK;
    for (int64_t e = (int64_t)blockIdx.x * BUILD_BLOCK + threadIdx.x; e < m; e += step) {
        const int32_t f = from[e];
        if (f != to[e] || (uint32_t)f >= (uint32_t)n) continue;
        if ((unsigned long long)__double_as_longlong(lat[e]) == selfMinBits[f]) atomicMax(&selfMinId[f], (int32_t)e);
    }
}

// ptr[0..n] = exclusive scan of cnt[0..n-1]; one workgroup.  A total of
// 2^31 - 1 or more sets BW_TOOBIG (the values are clamped and not used).
__global__ __launch_bounds__(BUILD_SCAN_BLOCK) void k_build_scan(const int32_t* __restrict__ cnt, int32_t n,
                                                                 int32_t* __restrict__ ptr, int32_t* __restrict__ W) {
    __shared__ long long part[BUILD_SCAN_BLOCK];
    const int t = (int)threadIdx.x;
    const int32_t chunk = (n + BUILD_SCAN_BLOCK - 1) / BUILD_SCAN_BLOCK;
    const int64_t lo = std::min<int64_t>((int64_t)t * chunk, n), hi = std::min<int64_t>(lo + chunk, n);
    long long s = 0;
    for (int64_t v = lo; v < hi; ++v) s += cnt[v];
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < BUILD_SCAN_BLOCK; d <<= 1) {                   // inclusive scan of the partial sums
        const long long x = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += x;
        __syncthreads();
    }
    long long acc = part[t] - s;
    for (int64_t v = lo; v < hi; ++v) {
        ptr[v] = (int32_t)std::min<long long>(acc, INT32_MAX);
        acc += cnt[v];
    }
    if (t == BUILD_SCAN_BLOCK - 1) {
        const long long total = part[t];
        ptr[n] = (int32_t)std::min<long long>(total, INT32_MAX);
        if (total >= (long long)INT32_MAX) W[BW_TOOBIG] = 1;
    }
}

// cursor[] / cursorIn[] start at zero; a row's slots are rowPtr[u] .. + count
__global__ __launch_bounds__(BUILD_BLOCK) void k_build_scatter(
    const int32_t* __restrict__ from, const int32_t* __restrict__ to, int64_t m, int32_t n, int32_t directed,
    const int32_t* __restrict__ rowPtr, const int32_t* __restrict__ inPtr, int32_t* __restrict__ cursor,
    int32_t* __restrict__ cursorIn, int32_t* __restrict__ nbr, int32_t* __restrict__ eid,
    int32_t* __restrict__ nbrIn, int32_t* __restrict__ eidIn) {
    const int lane = build_lane();
    const int64_t wave = (int64_t)blockIdx.x * (BUILD_BLOCK / 64) + (threadIdx.x >> 6);
    const int64_t step = (int64_t)gridDim.x * BUILD_BLOCK;
    for (int64_t base = wave * 64; base < m; base += step) {
        const int64_t e = base + lane;
        const bool in = e < m;
        const int32_t f = in ? from[e] : -1, t = in ? to[e] : -1;
        const bool arc = in && f != t && (uint32_t)f < (uint32_t)n && (uint32_t)t < (uint32_t)n;
        int headLane, runLen;
        wave_run(arc ? f : -1, headLane, runLen);
        int32_t s = (arc && headLane == lane) ? atomicAdd(&cursor[f], runLen) : 0;
        s = __shfl(s, headLane, 64) + (lane - headLane);
        if (!arc) continue;
        const int64_t a = (int64_t)rowPtr[f] + s;
        if (a < (int64_t)rowPtr[f + 1]) { nbr[a] = t; eid[a] = (int32_t)e; }
        if (directed) {
            const int64_t b = (int64_t)inPtr[t] + atomicAdd(&cursorIn[t], 1);
            if (b < (int64_t)inPtr[t + 1]) { nbrIn[b] = f; eidIn[b] = (int32_t)e; }
        } else {
            const int64_t b = (int64_t)rowPtr[t] + atomicAdd(&cursor[t], 1);
            if (b < (int64_t)rowPtr[t + 1]) { nbr[b] = f; eid[b] = (int32_t)e; }
        }
    }
}

// One workgroup per row of the CSR `ptr`.  sideMode 0: undirected out rows (an
// edge's arc out of its `from` is side 0, out of its `to` side 1); 1: directed
// out rows (side 0); 2: directed in rows (side 1).  LDS: bitmap[words] then
// prefix[words].  arcs / arc3 may be null (in rows).
__global__ __launch_bounds__(BUILD_BLOCK) void k_build_rows(
    const int32_t* __restrict__ ptr, const int32_t* __restrict__ nbr, const int32_t* __restrict__ eid,
    int32_t words, int32_t sideMode, const int32_t* __restrict__ from, const double* __restrict__ elat,
    const double* __restrict__ eloss, int32_t* __restrict__ col, double* __restrict__ lat,
    double* __restrict__ rel, Arc* __restrict__ arcs, Arc3* __restrict__ arc3, int32_t* __restrict__ epos,
    int32_t* __restrict__ W) {
    extern __shared__ uint32_t lds[];
    __shared__ uint32_t waveSum[BUILD_BLOCK / 64];
    uint32_t* bm = lds;
    uint32_t* pre = lds + words;
    const int32_t u = (int32_t)blockIdx.x;
    const int32_t b = ptr[u], deg = ptr[u + 1] - b;
    if (deg <= 0) return;                                              // uniform: before any barrier
    const int t = (int)threadIdx.x;
    for (int32_t w = t; w < words; w += BUILD_BLOCK) bm[w] = 0u;
    __syncthreads();
    bool dup = false;
    for (int32_t i = t; i < deg; i += BUILD_BLOCK) {
        const uint32_t v = (uint32_t)nbr[b + i];
        const uint32_t bit = 1u << (v & 31);
        if (atomicOr(&bm[v >> 5], bit) & bit) dup = true;
    }
    build_flag(dup, &W[BW_MULTI]);
    __syncthreads();
    // exclusive prefix popcount per word: a contiguous chunk per thread
    const int32_t chunk = (words + BUILD_BLOCK - 1) / BUILD_BLOCK;
    const int32_t w0 = min(t * chunk, words), w1 = min(w0 + chunk, words);
    uint32_t s = 0;
    for (int32_t w = w0; w < w1; ++w) s += (uint32_t)__popc(bm[w]);
    uint32_t inc = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t x = __shfl_up(inc, d, 64);
        if (build_lane() >= d) inc += x;
    }
    if (build_lane() == 63) waveSum[t >> 6] = inc;
    __syncthreads();
    uint32_t acc = inc - s;
    for (int k = 0; k < (t >> 6); ++k) acc += waveSum[k];
    for (int32_t w = w0; w < w1; ++w) {
        pre[w] = acc;
        acc += (uint32_t)__popc(bm[w]);
    }
    __syncthreads();
    for (int32_t i = t; i < deg; i += BUILD_BLOCK) {
        const uint32_t v = (uint32_t)nbr[b + i];
        const int32_t e = eid[b + i];
        const uint32_t rank = pre[v >> 5] + (uint32_t)__popc(bm[v >> 5] & ((1u << (v & 31)) - 1u));
        // (rank < the number of distinct neighbours <= deg: inside the row)
        const int64_t a = (int64_t)b + rank;
        const double L = elat[e], R = 1.0 - eloss[e];
        col[a] = (int32_t)v;
        lat[a] = L;
        rel[a] = R;
        if (arcs) {
            arcs[a].lat = L;
            arcs[a].col = (int32_t)v;
            const uint64_t bits = (uint64_t)__double_as_longlong(L);
            arc3[a] = Arc3{(int32_t)v, (uint32_t)bits, (uint32_t)(bits >> 32)};
        }
        const int32_t side = sideMode == 0 ? (from[e] == u ? 0 : 1) : sideMode - 1;
        epos[2 * (int64_t)e + side] = (int32_t)a;
    }
}

__global__ __launch_bounds__(BUILD_BLOCK) void k_build_link(const int32_t* __restrict__ from,
                                                            const int32_t* __restrict__ to, int64_t m,
                                                            int32_t directed, const int32_t* __restrict__ epos,
                                                            int32_t* __restrict__ outToIn, Arc* __restrict__ arcs) {
    const int64_t step = (int64_t)gridDim.x * BUILD_BLOCK;
    for (int64_t e = (int64_t)blockIdx.x * BUILD_BLOCK + threadIdx.x; e < m; e += step) {
        if (from[e] == to[e]) continue;
        const int32_t p = epos[2 * e], q = epos[2 * e + 1];
        outToIn[p] = q;
        arcs[p].pad = q;
        if (!directed) {
            outToIn[q] = p;
            arcs[q].pad = p;
        }
    }
}

__global__ __launch_bounds__(BUILD_BLOCK) void k_build_vfinal(
    int32_t n, int32_t directed, const int32_t* __restrict__ rowPtr, const int32_t* __restrict__ nSelf,
    const int32_t* __restrict__ selfNewest, const int32_t* __restrict__ selfMinId,
    const double* __restrict__ elat, const double* __restrict__ eloss, double* __restrict__ selfLat,
    double* __restrict__ selfRel, double* __restrict__ selfMinLat, double* __restrict__ selfMinRel,
    uint8_t* __restrict__ hasSelf, int32_t* __restrict__ edgeCount, int32_t* __restrict__ W) {
    const int32_t v = (int32_t)(blockIdx.x * BUILD_BLOCK + threadIdx.x);
    bool incomplete = false;
    if (v < n) {
        const int32_t ns = nSelf[v];
        double sl = 0.0, sr = 0.0, ml = 0.0, mr = 0.0;
        if (ns > 0) {
            const int32_t e = selfNewest[v], k = selfMinId[v];
            sl = elat[e];
            sr = 1.0 - eloss[e];
            ml = elat[k];
            mr = 1.0 - eloss[k];
        }
        selfLat[v] = sl; selfRel[v] = sr; selfMinLat[v] = ml; selfMinRel[v] = mr;
        hasSelf[v] = ns > 0 ? 1 : 0;
        long long c = (long long)(rowPtr[v + 1] - rowPtr[v]) + (directed ? (long long)ns : 2ll * ns);
        if (!directed && ns > 0) c -= 1;
        incomplete = c < (long long)n;
        edgeCount[v] = (int32_t)std::min<long long>(c, INT32_MAX);
        if (ns > 1) atomicMax(&W[BW_MAXSELF], ns);
    }
    build_flag(incomplete, &W[BW_INCOMPLETE]);
}

// ---- after a shard is configured ------------------------------------------
__global__ __launch_bounds__(BUILD_BLOCK) void k_build_heavy(const int32_t* __restrict__ rowPtr, int32_t n,
                                                             int32_t heavyDeg, uint32_t* __restrict__ bits) {
    const int32_t w = (int32_t)(blockIdx.x * BUILD_BLOCK + threadIdx.x);
    if (w >= (n + 31) / 32) return;
    uint32_t x = 0u;
    for (int k = 0; k < 32; ++k) {
        const int32_t v = w * 32 + k;
        if (v < n && rowPtr[v + 1] - rowPtr[v] >= heavyDeg) x |= 1u << k;
    }
    bits[w] = x;
}

__global__ __launch_bounds__(BUILD_BLOCK) void k_build_attached(const int32_t* __restrict__ attached, int32_t T,
                                                                int32_t n, uint8_t* __restrict__ isAttached) {
    const int32_t i = (int32_t)(blockIdx.x * BUILD_BLOCK + threadIdx.x);
    if (i < T && (uint32_t)attached[i] < (uint32_t)n) isAttached[attached[i]] = 1;
}

// ---- digests ----------------------------------------------------------------
__device__ __host__ inline uint64_t digest_mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
constexpr uint64_t DIGEST_K = 0x9e3779b97f4a7c15ull;

template <class T>
__global__ __launch_bounds__(BUILD_BLOCK) void k_array_digest(const T* __restrict__ p, int64_t count,
                                                              unsigned long long* __restrict__ acc) {
    const int64_t step = (int64_t)gridDim.x * BUILD_BLOCK;
    uint64_t h = 0;
    for (int64_t i = (int64_t)blockIdx.x * BUILD_BLOCK + threadIdx.x; i < count; i += step)
        h += digest_mix((uint64_t)p[i] ^ ((uint64_t)i * DIGEST_K));
    for (int d = 32; d >= 1; d >>= 1) h += __shfl_xor(h, d, 64);
    if (build_lane() == 0 && h != 0) atomicAdd(acc, (unsigned long long)h);
}

// ---- host side ------------------------------------------------------------------
#define BCHK(x)                                    \
    do {                                           \
        if ((x) != hipSuccess) return SHD_PE_EHIP; \
    } while (0)
#define BRC(x)               \
    do {                     \
        const int rc_ = (x); \
        if (rc_) return rc_; \
    } while (0)

void BuiltGraph::release() {
    if (!adopted && !allocs.empty()) {
        (void)hipSetDevice(device);
        for (void* p : allocs) (void)hipFree(p);
    }
    allocs.clear();
    dg = DevGraph{};
}

BuiltGraph::~BuiltGraph() { release(); }

namespace {

// the build's temporaries: freed with the object, their bytes counted
struct BuildRun {
    int device = 0;
    hipStream_t stream = nullptr;
    Stager stage;
    std::vector<void*> tmp;
    int64_t bytes = 0, peak = 0;
    int32_t* hW = nullptr;

    ~BuildRun() {
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
        for (void* p : tmp) (void)hipFree(p);
        if (hW) (void)hipHostFree(hW);
        if (stream) (void)hipStreamDestroy(stream);
    }
    template <class T>
    int alloc(T** p, size_t count) {
        const size_t b = std::max<size_t>(count, 1) * sizeof(T);
        if (hipMalloc((void**)p, b) != hipSuccess) { *p = nullptr; return SHD_PE_ENOMEM; }
        tmp.push_back(*p);
        bytes += (int64_t)b;
        peak = std::max(peak, bytes);
        return SHD_PE_OK;
    }
};

template <class T>
int out_alloc(BuiltGraph* g, T** p, size_t count) {
    const size_t b = std::max<size_t>(count * sizeof(T), 16);
    if (hipMalloc((void**)p, b) != hipSuccess) { *p = nullptr; return SHD_PE_ENOMEM; }
    g->allocs.push_back(*p);
    return SHD_PE_OK;
}

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

unsigned edge_grid(int64_t m) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((m + BUILD_BLOCK - 1) / BUILD_BLOCK, BUILD_MAX_GRID));
}

}  // namespace

#define BUILD_V(kernel, ...) hipLaunchKernelGGL(kernel, dim3(vGrid), dim3(BUILD_BLOCK), 0, r.stream, __VA_ARGS__)
#define BUILD_E(kernel, ...) hipLaunchKernelGGL(kernel, dim3(eGrid), dim3(BUILD_BLOCK), 0, r.stream, __VA_ARGS__)

int device_build_graph(const ShdPeGraphDesc* d, int device, int32_t maxN, HostGraph* g, BuiltGraph* out,
                       ShdPeBuildInfo* info) {
    if (!d || !g || !out || !info || d->nVertices <= 0 || d->nEdges < 0) return SHD_PE_EINVAL;
    if (d->nEdges > 0 && (!d->edgeFrom || !d->edgeTo || !d->edgeLatency || !d->edgePacketLoss))
        return SHD_PE_EINVAL;
    const int32_t n = d->nVertices;
    const int64_t m = d->nEdges;
    const int32_t directed = d->directed ? 1 : 0;
    // (edge ids travel as i32 through the scatter)
    if (n > maxN || m > (int64_t)INT32_MAX) {
        info->handedOff = 1;
        info->handOffWhy = 2;
        return SHD_PE_OK;
    }
    BCHK(hipSetDevice(device));
    out->device = device;
    BuildRun r;
    r.device = device;
    BCHK(hipStreamCreateWithFlags(&r.stream, hipStreamNonBlocking));
    r.stage.stream = r.stream;
    if (hipHostMalloc((void**)&r.hW, BW_COUNT * sizeof(int32_t)) != hipSuccess) { r.hW = nullptr; return SHD_PE_ENOMEM; }
    auto t0 = std::chrono::steady_clock::now();

    // ---- upload: 24 B per edge, once ----
    const size_t me = (size_t)m, nb = (size_t)n;
    int32_t *dFrom, *dTo, *dW;
    double *dLat, *dLoss, *dVloss = nullptr;
    BRC(r.alloc(&dFrom, me));
    BRC(r.alloc(&dTo, me));
    BRC(r.alloc(&dLat, me));
    BRC(r.alloc(&dLoss, me));
    BRC(r.alloc(&dW, (size_t)BW_COUNT));
    if (d->vertexPacketLoss) BRC(r.alloc(&dVloss, nb));
    BRC(r.stage.upload(dFrom, d->edgeFrom, me * 4));
    BRC(r.stage.upload(dTo, d->edgeTo, me * 4));
    BRC(r.stage.upload(dLat, d->edgeLatency, me * 8));
    BRC(r.stage.upload(dLoss, d->edgePacketLoss, me * 8));
    if (dVloss) BRC(r.stage.upload(dVloss, d->vertexPacketLoss, nb * 8));
    BCHK(hipMemsetAsync(dW, 0, BW_COUNT * sizeof(int32_t), r.stream));
    BCHK(hipStreamSynchronize(r.stream));
    info->msUpload = ms_since(t0);
    t0 = std::chrono::steady_clock::now();
    auto readW = [&]() -> int {
        BCHK(hipGetLastError());
        BCHK(hipMemcpyAsync(r.hW, dW, BW_COUNT * sizeof(int32_t), hipMemcpyDeviceToHost, r.stream));
        BCHK(hipStreamSynchronize(r.stream));
        return SHD_PE_OK;
    };
    // what ends the device part early: the temporaries' peak so far is reported
    auto hand_off = [&](int why) {
        info->handedOff = 1;
        info->handOffWhy = why;
        info->deviceBytesPeak = r.peak;
        info->msKernels = ms_since(t0);
        return SHD_PE_OK;
    };

    const unsigned vGrid = (unsigned)((nb + BUILD_BLOCK - 1) / BUILD_BLOCK);
    const unsigned eGrid = edge_grid(m);
    DevGraph& dg = out->dg;
    dg.n = n;

    // ---- per-vertex outputs, counts ----
    double *vrel, *selfLat, *selfRel, *selfMinLat, *selfMinRel;
    uint8_t* hasSelf;
    int32_t *rowPtr, *inPtr = nullptr;
    BRC(out_alloc(out, &vrel, nb));
    BRC(out_alloc(out, &selfLat, nb));
    BRC(out_alloc(out, &selfRel, nb));
    BRC(out_alloc(out, &selfMinLat, nb));
    BRC(out_alloc(out, &selfMinRel, nb));
    BRC(out_alloc(out, &hasSelf, nb));
    BRC(out_alloc(out, &rowPtr, nb + 1));
    if (directed) BRC(out_alloc(out, &inPtr, nb + 1));
    int32_t *cnt, *cntIn = nullptr, *nSelf, *selfNewest, *selfMinId, *edgeCount;
    unsigned long long* selfMinBits;
    BRC(r.alloc(&cnt, nb));
    if (directed) BRC(r.alloc(&cntIn, nb));
    BRC(r.alloc(&nSelf, nb));
    BRC(r.alloc(&selfNewest, nb));
    BRC(r.alloc(&selfMinId, nb));
    BRC(r.alloc(&selfMinBits, nb));
    BRC(r.alloc(&edgeCount, nb));
    BCHK(hipMemsetAsync(cnt, 0, nb * 4, r.stream));
    if (directed) BCHK(hipMemsetAsync(cntIn, 0, nb * 4, r.stream));
    BCHK(hipMemsetAsync(nSelf, 0, nb * 4, r.stream));
    BCHK(hipMemsetAsync(selfNewest, 0xff, nb * 4, r.stream));          // -1
    BCHK(hipMemsetAsync(selfMinId, 0xff, nb * 4, r.stream));
    BCHK(hipMemsetAsync(selfMinBits, 0xff, nb * 8, r.stream));

    BUILD_V(k_build_vertex, dVloss, n, vrel, dW);
    BUILD_E(k_build_count, dFrom, dTo, dLat, dLoss, m, n, directed, cnt, cntIn, nSelf, selfNewest, selfMinBits, dW);
    hipLaunchKernelGGL(k_build_scan, dim3(1), dim3(BUILD_SCAN_BLOCK), 0, r.stream, cnt, n, rowPtr, dW);
    if (directed)
        hipLaunchKernelGGL(k_build_scan, dim3(1), dim3(BUILD_SCAN_BLOCK), 0, r.stream, cntIn, n, inPtr, dW);
    BRC(readW());
    if (r.hW[BW_ERR] || r.hW[BW_TOOBIG]) return SHD_PE_EINVAL;
    if (r.hW[BW_ANYSELF]) BUILD_E(k_build_selfmin, dFrom, dTo, dLat, m, n, selfMinBits, selfMinId);
    int32_t nArcs32 = 0;
    BCHK(hipMemcpyAsync(&r.hW[BW_COUNT - 1], rowPtr + n, 4, hipMemcpyDeviceToHost, r.stream));
    BCHK(hipStreamSynchronize(r.stream));
    nArcs32 = r.hW[BW_COUNT - 1];
    const size_t nArcs = (size_t)nArcs32;

    // ---- scatter, rows, link ----
    int32_t *col, *outToIn, *inCol = nullptr;
    double *lat, *rel, *inLat = nullptr, *inRel = nullptr;
    Arc* arcs;
    Arc3* arc3;
    BRC(out_alloc(out, &col, nArcs));
    BRC(out_alloc(out, &lat, nArcs));
    BRC(out_alloc(out, &rel, nArcs));
    BRC(out_alloc(out, &outToIn, nArcs));
    BRC(out_alloc(out, &arcs, nArcs));
    BRC(out_alloc(out, &arc3, nArcs));
    if (directed) {
        BRC(out_alloc(out, &inCol, nArcs));
        BRC(out_alloc(out, &inLat, nArcs));
        BRC(out_alloc(out, &inRel, nArcs));
    }
    int32_t *nbr, *eid, *nbrIn = nullptr, *eidIn = nullptr, *epos;
    BRC(r.alloc(&nbr, nArcs));
    BRC(r.alloc(&eid, nArcs));
    if (directed) {
        BRC(r.alloc(&nbrIn, nArcs));
        BRC(r.alloc(&eidIn, nArcs));
    }
    BRC(r.alloc(&epos, 2 * me));
    // the counts become the cursors
    BCHK(hipMemsetAsync(cnt, 0, nb * 4, r.stream));
    if (directed) BCHK(hipMemsetAsync(cntIn, 0, nb * 4, r.stream));
    BUILD_E(k_build_scatter, dFrom, dTo, m, n, directed, rowPtr, inPtr, cnt, cntIn, nbr, eid, nbrIn, eidIn);
    const int32_t words = (n + 31) / 32;
    const size_t lds = (size_t)words * 8;                              // <= 32 KiB at BUILD_MAX_N
    hipLaunchKernelGGL(k_build_rows, dim3((unsigned)n), dim3(BUILD_BLOCK), lds, r.stream, rowPtr, nbr, eid, words,
                       directed ? 1 : 0, dFrom, dLat, dLoss, col, lat, rel, arcs, arc3, epos, dW);
    if (directed)
        hipLaunchKernelGGL(k_build_rows, dim3((unsigned)n), dim3(BUILD_BLOCK), lds, r.stream, inPtr, nbrIn, eidIn,
                           words, 2, dFrom, dLat, dLoss, inCol, inLat, inRel, (Arc*)nullptr, (Arc3*)nullptr, epos,
                           dW);
    BRC(readW());
    if (r.hW[BW_MULTI]) return hand_off(1);                            // `out` frees what was made
    BUILD_E(k_build_link, dFrom, dTo, m, directed, epos, outToIn, arcs);
    BUILD_V(k_build_vfinal, n, directed, rowPtr, nSelf, selfNewest, selfMinId, dLat, dLoss, selfLat, selfRel,
            selfMinLat, selfMinRel, hasSelf, edgeCount, dW);
    BRC(readW());
    info->msKernels = ms_since(t0);
    t0 = std::chrono::steady_clock::now();

    dg.rowPtr = rowPtr; dg.col = col; dg.lat = lat; dg.rel = rel; dg.arcs = arcs; dg.arc3 = arc3;
    dg.outToIn = outToIn;
    dg.vrel = vrel; dg.selfLat = selfLat; dg.selfRel = selfRel; dg.hasSelf = hasSelf;
    dg.selfMinLat = selfMinLat; dg.selfMinRel = selfMinRel;
    if (directed) { dg.inPtr = inPtr; dg.inCol = inCol; dg.inLat = inLat; dg.inRel = inRel; }
    else { dg.inPtr = rowPtr; dg.inCol = col; dg.inLat = lat; dg.inRel = rel; }

    // ---- read-back: HostGraph as build_host_graph leaves it ----
    g->n = n;
    g->directed = directed;
    g->nEdges = m;
    g->latFold = false;
    g->isComplete = r.hW[BW_INCOMPLETE] == 0;
    g->rowPtr.resize(nb + 1);
    g->col.resize(nArcs); g->lat.resize(nArcs); g->rel.resize(nArcs); g->outToIn.resize(nArcs);
    g->vrel.resize(nb); g->selfLat.resize(nb); g->selfRel.resize(nb);
    g->selfMinLat.resize(nb); g->selfMinRel.resize(nb); g->hasSelf.resize(nb);
    BRC(r.stage.download(g->rowPtr.data(), rowPtr, (nb + 1) * 4));
    BRC(r.stage.download(g->col.data(), col, nArcs * 4));
    BRC(r.stage.download(g->lat.data(), lat, nArcs * 8));
    BRC(r.stage.download(g->rel.data(), rel, nArcs * 8));
    BRC(r.stage.download(g->outToIn.data(), outToIn, nArcs * 4));
    if (directed) {
        g->inPtr.resize(nb + 1);
        g->inCol.resize(nArcs); g->inLat.resize(nArcs); g->inRel.resize(nArcs);
        BRC(r.stage.download(g->inPtr.data(), inPtr, (nb + 1) * 4));
        BRC(r.stage.download(g->inCol.data(), inCol, nArcs * 4));
        BRC(r.stage.download(g->inLat.data(), inLat, nArcs * 8));
        BRC(r.stage.download(g->inRel.data(), inRel, nArcs * 8));
    }
    BRC(r.stage.download(g->vrel.data(), vrel, nb * 8));
    BRC(r.stage.download(g->selfLat.data(), selfLat, nb * 8));
    BRC(r.stage.download(g->selfRel.data(), selfRel, nb * 8));
    BRC(r.stage.download(g->selfMinLat.data(), selfMinLat, nb * 8));
    BRC(r.stage.download(g->selfMinRel.data(), selfMinRel, nb * 8));
    BRC(r.stage.download(g->hasSelf.data(), hasSelf, nb));
    if (r.hW[BW_MAXSELF] > 1) {                                        // several loops on a vertex: a multigraph
        g->edgeCount.resize(nb);
        BRC(r.stage.download(g->edgeCount.data(), edgeCount, nb * 4));
    }
    arc_latency_stats(g);
    info->msReadback = ms_since(t0);
    info->deviceBytesPeak = r.peak;
    return SHD_PE_OK;
}

int finish_built_graph(const std::vector<int32_t>& attached, int32_t heavyDeg, void* stream, DevGraph* dg,
                       std::vector<void*>* allocs) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int32_t n = dg->n, T = (int32_t)attached.size();
    const size_t hw = ((size_t)n + 31) / 32;
    int32_t* dAtt;
    uint8_t* dIs;
    uint32_t* dHeavy;
    auto alloc = [&](auto** p, size_t bytes) {
        if (hipMalloc((void**)p, std::max<size_t>(bytes, 16)) != hipSuccess) { *p = nullptr; return SHD_PE_ENOMEM; }
        allocs->push_back(*p);
        return SHD_PE_OK;
    };
    BRC(alloc(&dAtt, (size_t)T * 4));
    BRC(alloc(&dIs, (size_t)n));
    BRC(alloc(&dHeavy, hw * 4));
    if (T > 0) BCHK(hipMemcpyAsync(dAtt, attached.data(), (size_t)T * 4, hipMemcpyHostToDevice, st));
    BCHK(hipMemsetAsync(dIs, 0, (size_t)n, st));
    if (T > 0)
        hipLaunchKernelGGL(k_build_attached, dim3((unsigned)((T + BUILD_BLOCK - 1) / BUILD_BLOCK)), dim3(BUILD_BLOCK),
                           0, st, dAtt, T, n, dIs);
    hipLaunchKernelGGL(k_build_heavy, dim3((unsigned)((hw + BUILD_BLOCK - 1) / BUILD_BLOCK)), dim3(BUILD_BLOCK), 0, st,
                       dg->rowPtr, n, heavyDeg, dHeavy);
    BCHK(hipGetLastError());
    BCHK(hipStreamSynchronize(st));
    dg->T = T;
    dg->attached = dAtt;
    dg->isAttached = dIs;
    dg->heavyBits = dHeavy;
    return SHD_PE_OK;
}

int device_array_digest(const void* p, int width, int64_t count, uint64_t* dAcc, void* stream, uint64_t* out) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    *out = 0;
    if (!p || count <= 0) return SHD_PE_OK;
    BCHK(hipMemsetAsync(dAcc, 0, 8, st));
    const unsigned eGrid = edge_grid(count);
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(dAcc);
    if (width == 1) hipLaunchKernelGGL(k_array_digest<uint8_t>, dim3(eGrid), dim3(BUILD_BLOCK), 0, st, (const uint8_t*)p, count, acc);
    else if (width == 4) hipLaunchKernelGGL(k_array_digest<uint32_t>, dim3(eGrid), dim3(BUILD_BLOCK), 0, st, (const uint32_t*)p, count, acc);
    else if (width == 8) hipLaunchKernelGGL(k_array_digest<uint64_t>, dim3(eGrid), dim3(BUILD_BLOCK), 0, st, (const uint64_t*)p, count, acc);
    else return SHD_PE_EINVAL;
    BCHK(hipGetLastError());
    BCHK(hipMemcpyAsync(out, dAcc, 8, hipMemcpyDeviceToHost, st));
    BCHK(hipStreamSynchronize(st));
    return SHD_PE_OK;
}

uint64_t host_array_digest(const void* p, int width, int64_t count) {
    uint64_t h = 0;
    for (int64_t i = 0; i < count; ++i) {
        uint64_t bits = 0;
        std::memcpy(&bits, (const char*)p + (size_t)i * (size_t)width, (size_t)width);   // little-endian zero-extension
        h += digest_mix(bits ^ ((uint64_t)i * DIGEST_K));
    }
    return h;
}

}  // namespace shdpe
