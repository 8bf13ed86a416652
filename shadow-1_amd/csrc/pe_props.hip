// pe_props.hip -- graph property check on the device.
//
//   shd_pe_graph_props   _topology_checkGraphProperties        topology.c:724-809
//     k_props_count / k_props_complete   _topology_isComplete           :450-552
//     undirected: k_props_hook / k_props_jump      igraph_clusters (weak) :745
//     directed:   trim / pivot / colouring kernels igraph_clusters (STRONG) :745
//
// The host prepares nothing: edgeFrom / edgeTo are uploaded as given (8 B per
// edge) and every kernel is edge-parallel (a grid-stride loop over the edge
// list) or vertex-parallel over n-sized arrays.  No CSR on either side.
//
// Undirected clusters: min-label hooking over the edges (labels read first,
// atomicMin only where it improves) alternating with pointer jumping, to the
// fixpoint "every edge has equal labels and every label is its own label";
// labels only fall and stay inside the component, so the fixpoint label is the
// component's smallest id.
//
// Directed clusters: the multistep scheme over a live mask.
//   trim      live vertices without a live in-arc or without a live out-arc
//             (self-loops aside) are their own cluster; repeated to a fixpoint;
//   pivot     the live vertex of largest count: forward and backward reach by
//             edge sweeps, the intersection is one cluster (its id: a min
//             reduction);
//   colouring colour = own id, the minimum colour pushed forward over live
//             arcs to a fixpoint; colour[v] == v marks a root (no smaller
//             vertex reaches it); reaching backward from every root inside its
//             colour class gives the root's cluster, whose smallest id is the
//             root.  Remove, trim, repeat until nothing is live.
// Reach sweeps are stamped with the sweep's generation (a mark fires only if
// it is older than the running sweep), so one sweep advances a frontier by
// exactly one arc whatever the schedule.  Clusters and their minimum ids are
// unique, so no result depends on scheduling.
//
// Ordering: kernel boundaries on one stream, nothing else.  A sweep reports
// "changed" with one store per wave into a device word the host reads every
// few sweeps.  All stores are vector stores from plain C++.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdlib>
#include <cstring>

#include "pe_stage.hpp"
#include "shd_pathengine.h"

namespace shdpe {

// control words on the device (one 64-B block, read back whole)
enum { W_ERR = 0, W_CHANGED, W_LIVE, W_FIRSTINC, W_MINID, W_CLUSTERS, W_LARGEST, W_PAD, W_PIVOT /* u64 */, W_COUNT = 16 };

constexpr int PROPS_BLOCK = 256;
constexpr int PROPS_MAX_GRID = 2048;
// the sweep count at which the device form's time at the C5 shape passes the host form's there
// (profiles/graph_props.json): 2.10 ms / 7.19 us per sweep
constexpr int32_t PROPS_DEFAULT_BUDGET = 292;

__device__ __forceinline__ int props_lane() { return (int)(threadIdx.x & 63); }

// one store per wave in which any lane saw a change
__device__ __forceinline__ void wave_flag(bool ch, int32_t* word) {
    const unsigned long long b = __ballot(ch);
    if (b != 0ull && props_lane() == (int)__ffsll((long long)b) - 1) *word = 1;
}

__device__ __forceinline__ int32_t wave_min(int32_t x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = min(x, __shfl_xor(x, o, 64));
    return x;
}

// ---- completeness ----------------------------------------------------------
// cnt[from] += 1 per edge; undirected also cnt[to] += 1 (a self-loop counts
// twice) and hasSelf[v] = 1.  A bad endpoint sets W_ERR and is skipped.
// RUNS: GraphML lists a complete graph's edges grouped by source, so a wave
// holds long runs of one `from`: each run is counted inside the wave (ballot
// of the run heads) and issues one atomic.
template <bool RUNS>
__global__ __launch_bounds__(PROPS_BLOCK) void k_props_count(const int32_t* __restrict__ from,
                                                             const int32_t* __restrict__ to, int64_t m,
                                                             int32_t n, int32_t directed,
                                                             int32_t* __restrict__ cnt,
                                                             uint8_t* __restrict__ hasSelf,
                                                             int32_t* __restrict__ W) {
    const int lane = props_lane();
    const int64_t wave = (int64_t)blockIdx.x * (PROPS_BLOCK / 64) + (threadIdx.x >> 6);
    const int64_t step = (int64_t)gridDim.x * PROPS_BLOCK;
    bool bad = false;
    for (int64_t base = wave * 64; base < m; base += step) {          // uniform per wave
        const int64_t e = base + lane;
        const bool in = e < m;
        const int32_t f = in ? from[e] : -1, t = in ? to[e] : -1;
        const bool ok = in && (uint32_t)f < (uint32_t)n && (uint32_t)t < (uint32_t)n;
        bad = bad || (in && !ok);
        if (RUNS) {
            const int32_t key = ok ? f : -1;
            const int32_t prev = __shfl_up(key, 1, 64);
            const bool head = lane == 0 || key != prev;
            const unsigned long long hb = __ballot(head);
            const unsigned long long above = hb & ~((2ull << lane) - 1ull);   // heads past this lane
            const int next = above ? (int)__ffsll((long long)above) - 1 : 64;
            if (head && key >= 0) atomicAdd(&cnt[key], next - lane);
        } else if (ok) {
            atomicAdd(&cnt[f], 1);
        }
        if (ok && !directed) {
            atomicAdd(&cnt[t], 1);
            if (f == t) hasSelf[f] = 1;
        }
    }
    wave_flag(bad, &W[W_ERR]);
}

// corrected count against n; W_FIRSTINC = lowest failing vertex
__global__ __launch_bounds__(PROPS_BLOCK) void k_props_complete(const int32_t* __restrict__ cnt,
                                                                const uint8_t* __restrict__ hasSelf, int32_t n,
                                                                int32_t* __restrict__ W) {
    const int32_t v = (int32_t)(blockIdx.x * PROPS_BLOCK + threadIdx.x);
    int32_t bad = INT_MAX;
    if (v < n && cnt[v] - (int32_t)hasSelf[v] < n) bad = v;
    bad = wave_min(bad);
    if (props_lane() == 0 && bad != INT_MAX) atomicMin(&W[W_FIRSTINC], bad);
}

// ---- undirected: hooking + pointer jumping ---------------------------------
__global__ __launch_bounds__(PROPS_BLOCK) void k_props_iota(int32_t* __restrict__ L, int32_t n) {
    const int32_t v = (int32_t)(blockIdx.x * PROPS_BLOCK + threadIdx.x);
    if (v < n) L[v] = v;
}

__global__ __launch_bounds__(PROPS_BLOCK) void k_props_hook(const int32_t* __restrict__ from,
                                                            const int32_t* __restrict__ to, int64_t m,
                                                            int32_t* __restrict__ L, int32_t* __restrict__ W) {
    const int64_t step = (int64_t)gridDim.x * PROPS_BLOCK;
    bool ch = false;
    for (int64_t e = (int64_t)blockIdx.x * PROPS_BLOCK + threadIdx.x; e < m; e += step) {
        const int32_t u = from[e], v = to[e];
        const int32_t a = L[u], b = L[v];
        if (a == b) continue;
        ch = true;
        // the smaller label goes to the other endpoint and to its label's vertex
        if (a < b) { atomicMin(&L[v], a); atomicMin(&L[b], a); }
        else { atomicMin(&L[u], b); atomicMin(&L[a], b); }
    }
    wave_flag(ch, &W[W_CHANGED]);
}

__global__ __launch_bounds__(PROPS_BLOCK) void k_props_jump(int32_t* __restrict__ L, int32_t n,
                                                            int32_t* __restrict__ W) {
    const int32_t v = (int32_t)(blockIdx.x * PROPS_BLOCK + threadIdx.x);
    bool ch = false;
    if (v < n) {
        const int32_t l0 = L[v];
        int32_t l = l0;
#pragma unroll
        for (int k = 0; k < 4; ++k) l = L[l];            // labels only fall: any value read is valid
        if (l != l0) { L[v] = l; ch = true; }
    }
    wave_flag(ch, &W[W_CHANGED]);
}

// ---- directed: trim / pivot / colouring -------------------------------------
__global__ __launch_bounds__(PROPS_BLOCK) void k_props_dir_init(int32_t* __restrict__ M, uint8_t* __restrict__ live,
                                                                int32_t n) {
    const int32_t v = (int32_t)(blockIdx.x * PROPS_BLOCK + threadIdx.x);
    if (v < n) { M[v] = -1; live[v] = 1; }
}

__global__ __launch_bounds__(PROPS_BLOCK) void k_props_trim_mark(const int32_t* __restrict__ from,
                                                                 const int32_t* __restrict__ to, int64_t m,
                                                                 const uint8_t* __restrict__ live,
                                                                 uint8_t* __restrict__ inMark,
                                                                 uint8_t* __restrict__ outMark) {
    const int64_t step = (int64_t)gridDim.x * PROPS_BLOCK;
    for (int64_t e = (int64_t)blockIdx.x * PROPS_BLOCK + threadIdx.x; e < m; e += step) {
        const int32_t u = from[e], v = to[e];
        if (u == v || !live[u] || !live[v]) continue;
        outMark[u] = 1;                                   // same-value races are benign
        inMark[v] = 1;
    }
}

// a live vertex missing either mark is its own cluster; the marks are cleared
// for the next trim
__global__ __launch_bounds__(PROPS_BLOCK) void k_props_trim_apply(uint8_t* __restrict__ live,
                                                                  uint8_t* __restrict__ inMark,
                                                                  uint8_t* __restrict__ outMark,
                                                                  int32_t* __restrict__ M, int32_t n,
                                                                  int32_t* __restrict__ W) {
    const int32_t v = (int32_t)(blockIdx.x * PROPS_BLOCK + threadIdx.x);
    bool gone = false;
    if (v < n) {
        gone = live[v] && !(inMark[v] && outMark[v]);
        inMark[v] = 0;
        outMark[v] = 0;
        if (gone) { live[v] = 0; M[v] = v; }
    }
    const unsigned long long b = __ballot(gone);
    if (b != 0ull && props_lane() == 0) {
        atomicSub(&W[W_LIVE], (int32_t)__popcll(b));
        W[W_CHANGED] = 1;
    }
}

// pivot: the live vertex with the largest count, the smallest id among equals
__global__ __launch_bounds__(PROPS_BLOCK) void k_props_pivot_pick(const uint8_t* __restrict__ live,
                                                                  const int32_t* __restrict__ cnt, int32_t n,
                                                                  int32_t* __restrict__ W) {
    const int32_t v = (int32_t)(blockIdx.x * PROPS_BLOCK + threadIdx.x);
    unsigned long long key = 0ull;                        // 0 = no live vertex in this lane
    if (v < n && live[v])
        key = ((unsigned long long)(uint32_t)cnt[v] << 32) | (uint32_t)(INT_MAX - v);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long ok = __shfl_xor(key, o, 64);
        key = ok > key ? ok : key;
    }
    if (props_lane() == 0 && key != 0ull) atomicMax((unsigned long long*)&W[W_PIVOT], key);
}

__global__ void k_props_pivot_seed(const int32_t* __restrict__ W, int32_t* __restrict__ fw,
                                   int32_t* __restrict__ bw, int32_t n) {
    const unsigned long long key = *(const unsigned long long*)&W[W_PIVOT];
    const int32_t p = INT_MAX - (int32_t)(uint32_t)(key & 0xffffffffull);
    if (threadIdx.x == 0 && blockIdx.x == 0 && key != 0ull && p >= 0 && p < n) { fw[p] = 1; bw[p] = 1; }
}

// one arc further in both directions: a mark of an earlier sweep (0 < mark <
// gen) fires, the new mark is gen
__global__ __launch_bounds__(PROPS_BLOCK) void k_props_reach(const int32_t* __restrict__ from,
                                                             const int32_t* __restrict__ to, int64_t m,
                                                             const uint8_t* __restrict__ live,
                                                             int32_t* __restrict__ fw, int32_t* __restrict__ bw,
                                                             int32_t gen, int32_t* __restrict__ W) {
    const int64_t step = (int64_t)gridDim.x * PROPS_BLOCK;
    bool ch = false;
    for (int64_t e = (int64_t)blockIdx.x * PROPS_BLOCK + threadIdx.x; e < m; e += step) {
        const int32_t u = from[e], v = to[e];
        if (u == v || !live[u] || !live[v]) continue;
        const int32_t fu = fw[u], bv = bw[v];
        if (fu != 0 && fu < gen && fw[v] == 0) { fw[v] = gen; ch = true; }
        if (bv != 0 && bv < gen && bw[u] == 0) { bw[u] = gen; ch = true; }
    }
    wave_flag(ch, &W[W_CHANGED]);
}

__global__ __launch_bounds__(PROPS_BLOCK) void k_props_pivot_min(const uint8_t* __restrict__ live,
                                                                 const int32_t* __restrict__ fw,
                                                                 const int32_t* __restrict__ bw, int32_t n,
                                                                 int32_t* __restrict__ W) {
    const int32_t v = (int32_t)(blockIdx.x * PROPS_BLOCK + threadIdx.x);
    int32_t id = INT_MAX;
    if (v < n && live[v] && fw[v] && bw[v]) id = v;
    id = wave_min(id);
    if (props_lane() == 0 && id != INT_MAX) atomicMin(&W[W_MINID], id);
}

__global__ __launch_bounds__(PROPS_BLOCK) void k_props_pivot_apply(uint8_t* __restrict__ live,
                                                                   const int32_t* __restrict__ fw,
                                                                   const int32_t* __restrict__ bw,
                                                                   int32_t* __restrict__ M, int32_t n,
                                                                   int32_t* __restrict__ W) {
    const int32_t v = (int32_t)(blockIdx.x * PROPS_BLOCK + threadIdx.x);
    const int32_t id = W[W_MINID];
    const bool in = v < n && live[v] && fw[v] && bw[v];
    if (in) { M[v] = id; live[v] = 0; }
    const unsigned long long b = __ballot(in);
    if (b != 0ull && props_lane() == 0) atomicSub(&W[W_LIVE], (int32_t)__popcll(b));
}

__global__ __launch_bounds__(PROPS_BLOCK) void k_props_colour_init(const uint8_t* __restrict__ live,
                                                                   int32_t* __restrict__ colour, int32_t n) {
    const int32_t v = (int32_t)(blockIdx.x * PROPS_BLOCK + threadIdx.x);
    if (v < n) colour[v] = live[v] ? v : INT_MAX;
}

__global__ __launch_bounds__(PROPS_BLOCK) void k_props_colour_push(const int32_t* __restrict__ from,
                                                                   const int32_t* __restrict__ to, int64_t m,
                                                                   const uint8_t* __restrict__ live,
                                                                   int32_t* __restrict__ colour,
                                                                   int32_t* __restrict__ W) {
    const int64_t step = (int64_t)gridDim.x * PROPS_BLOCK;
    bool ch = false;
    for (int64_t e = (int64_t)blockIdx.x * PROPS_BLOCK + threadIdx.x; e < m; e += step) {
        const int32_t u = from[e], v = to[e];
        if (u == v || !live[u] || !live[v]) continue;
        const int32_t cu = colour[u];
        if (cu < colour[v]) { atomicMin(&colour[v], cu); ch = true; }
    }
    wave_flag(ch, &W[W_CHANGED]);
}

__global__ __launch_bounds__(PROPS_BLOCK) void k_props_back_init(const uint8_t* __restrict__ live,
                                                                 const int32_t* __restrict__ colour,
                                                                 int32_t* __restrict__ reached, int32_t n) {
    const int32_t v = (int32_t)(blockIdx.x * PROPS_BLOCK + threadIdx.x);
    if (v < n) reached[v] = live[v] && colour[v] == v;
}

// backward from the roots, inside the colour class
__global__ __launch_bounds__(PROPS_BLOCK) void k_props_back(const int32_t* __restrict__ from,
                                                            const int32_t* __restrict__ to, int64_t m,
                                                            const uint8_t* __restrict__ live,
                                                            const int32_t* __restrict__ colour,
                                                            int32_t* __restrict__ reached, int32_t* __restrict__ W) {
    const int64_t step = (int64_t)gridDim.x * PROPS_BLOCK;
    bool ch = false;
    for (int64_t e = (int64_t)blockIdx.x * PROPS_BLOCK + threadIdx.x; e < m; e += step) {
        const int32_t u = from[e], v = to[e];
        if (u == v || !live[u] || !live[v]) continue;
        if (reached[v] && !reached[u] && colour[u] == colour[v]) { reached[u] = 1; ch = true; }
    }
    wave_flag(ch, &W[W_CHANGED]);
}

__global__ __launch_bounds__(PROPS_BLOCK) void k_props_colour_apply(uint8_t* __restrict__ live,
                                                                    const int32_t* __restrict__ reached,
                                                                    const int32_t* __restrict__ colour,
                                                                    int32_t* __restrict__ M, int32_t n,
                                                                    int32_t* __restrict__ W) {
    const int32_t v = (int32_t)(blockIdx.x * PROPS_BLOCK + threadIdx.x);
    const bool in = v < n && live[v] && reached[v];
    if (in) { M[v] = colour[v]; live[v] = 0; }
    const unsigned long long b = __ballot(in);
    if (b != 0ull && props_lane() == 0) atomicSub(&W[W_LIVE], (int32_t)__popcll(b));
}

// ---- summary ---------------------------------------------------------------
__global__ __launch_bounds__(PROPS_BLOCK) void k_props_sizes(const int32_t* __restrict__ M,
                                                             int32_t* __restrict__ size, int32_t n) {
    const int32_t v = (int32_t)(blockIdx.x * PROPS_BLOCK + threadIdx.x);
    if (v >= n) return;
    const int32_t l = M[v];
    if ((uint32_t)l < (uint32_t)n) atomicAdd(&size[l], 1);     // every vertex has a label by now
}

__global__ __launch_bounds__(PROPS_BLOCK) void k_props_summary(const int32_t* __restrict__ M,
                                                               const int32_t* __restrict__ size, int32_t n,
                                                               int32_t* __restrict__ W) {
    const int32_t v = (int32_t)(blockIdx.x * PROPS_BLOCK + threadIdx.x);
    const bool root = v < n && M[v] == v;
    int32_t big = root ? size[v] : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) big = max(big, __shfl_xor(big, o, 64));
    const unsigned long long b = __ballot(root);
    if (b != 0ull && props_lane() == 0) {
        atomicAdd(&W[W_CLUSTERS], (int32_t)__popcll(b));
        atomicMax(&W[W_LARGEST], big);
    }
}

// ---- host side ---------------------------------------------------------------
struct PropsRun {
    int32_t device = 0, n = 0;
    int64_t m = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    Stager stage;                             // the edge endpoints' way up (pe_stage.hpp)
    int32_t *dFrom = nullptr, *dTo = nullptr;
    int32_t *dCnt = nullptr, *dM = nullptr, *dA = nullptr, *dB = nullptr, *dW = nullptr;
    uint8_t *dSelf = nullptr, *dLive = nullptr, *dIn = nullptr, *dOut = nullptr;
    int32_t* hW = nullptr;                    // page-locked mirror of dW
    int64_t sweeps = 0, rounds = 0, budget = 0;
    bool handOff = false;
    unsigned vGrid = 1, eGrid = 1;

    ~PropsRun() {
        if (!stream) return;
        (void)hipSetDevice(device);
        (void)hipStreamSynchronize(stream);
        for (void* p : {(void*)dFrom, (void*)dTo, (void*)dCnt, (void*)dM, (void*)dA, (void*)dB, (void*)dW,
                        (void*)dSelf, (void*)dLive, (void*)dIn, (void*)dOut})
            if (p) (void)hipFree(p);
        if (hW) (void)hipHostFree(hW);
        for (hipEvent_t e : {ev0, ev1})
            if (e) (void)hipEventDestroy(e);
        (void)hipStreamDestroy(stream);
    }
};

#define PRCHK(x)                                   \
    do {                                           \
        if ((x) != hipSuccess) return SHD_PE_EHIP; \
    } while (0)
#define PRRC(x)              \
    do {                     \
        const int rc_ = (x); \
        if (rc_) return rc_; \
    } while (0)

template <class T>
static int props_alloc(T** p, size_t count) {
    if (hipMalloc((void**)p, std::max<size_t>(count, 1) * sizeof(T)) != hipSuccess) {
        *p = nullptr;
        return SHD_PE_ENOMEM;
    }
    return SHD_PE_OK;
}

static int props_read(PropsRun& r) {
    PRCHK(hipMemcpyAsync(r.hW, r.dW, W_COUNT * sizeof(int32_t), hipMemcpyDeviceToHost, r.stream));
    PRCHK(hipStreamSynchronize(r.stream));
    return SHD_PE_OK;
}

// Runs `step` (one edge sweep plus its vertex kernels) until a batch of steps
// changes nothing; the changed word is read once per batch of 1, 2, 4, 4, ...
// steps.  Returns 1 when the sweep budget ran out first.
template <class Step>
static int props_fixpoint(PropsRun& r, Step step) {
    int batch = 1;
    for (;;) {
        PRCHK(hipMemsetAsync(&r.dW[W_CHANGED], 0, sizeof(int32_t), r.stream));
        for (int k = 0; k < batch; ++k) {
            if (r.sweeps >= r.budget) { r.handOff = true; return 1; }
            ++r.sweeps;
            step();
        }
        PRCHK(hipGetLastError());
        PRRC(props_read(r));
        if (!r.hW[W_CHANGED]) return SHD_PE_OK;
        batch = std::min(batch * 2, 4);
    }
}

#define PROPS_V(kernel, ...) hipLaunchKernelGGL(kernel, dim3(r.vGrid), dim3(PROPS_BLOCK), 0, r.stream, __VA_ARGS__)
#define PROPS_E(kernel, ...) hipLaunchKernelGGL(kernel, dim3(r.eGrid), dim3(PROPS_BLOCK), 0, r.stream, __VA_ARGS__)

static int props_undirected(PropsRun& r) {
    PROPS_V(k_props_iota, r.dM, r.n);
    const int rc = props_fixpoint(r, [&] {
        ++r.rounds;
        PROPS_E(k_props_hook, r.dFrom, r.dTo, r.m, r.dM, r.dW);
        PROPS_V(k_props_jump, r.dM, r.n, r.dW);
    });
    return rc;
}

static int props_trim(PropsRun& r) {
    ++r.rounds;
    return props_fixpoint(r, [&] {
        PROPS_E(k_props_trim_mark, r.dFrom, r.dTo, r.m, r.dLive, r.dIn, r.dOut);
        PROPS_V(k_props_trim_apply, r.dLive, r.dIn, r.dOut, r.dM, r.n, r.dW);
    });
}

static int props_directed(PropsRun& r) {
    const size_t nb = (size_t)r.n;
    PROPS_V(k_props_dir_init, r.dM, r.dLive, r.n);
    PRCHK(hipMemsetAsync(r.dIn, 0, nb, r.stream));
    PRCHK(hipMemsetAsync(r.dOut, 0, nb, r.stream));
    int rc = props_trim(r);                               // leaves W_LIVE in hW
    if (rc) return rc;
    bool pivot = true;
    while (r.hW[W_LIVE] > 0) {
        ++r.rounds;
        if (pivot) {
            pivot = false;
            PRCHK(hipMemsetAsync(r.dA, 0, nb * 4, r.stream));
            PRCHK(hipMemsetAsync(r.dB, 0, nb * 4, r.stream));
            PROPS_V(k_props_pivot_pick, r.dLive, r.dCnt, r.n, r.dW);
            hipLaunchKernelGGL(k_props_pivot_seed, dim3(1), dim3(64), 0, r.stream, r.dW, r.dA, r.dB, r.n);
            int32_t gen = 1;
            rc = props_fixpoint(r, [&] {
                ++gen;
                PROPS_E(k_props_reach, r.dFrom, r.dTo, r.m, r.dLive, r.dA, r.dB, gen, r.dW);
            });
            if (rc) return rc;
            PROPS_V(k_props_pivot_min, r.dLive, r.dA, r.dB, r.n, r.dW);
            PROPS_V(k_props_pivot_apply, r.dLive, r.dA, r.dB, r.dM, r.n, r.dW);
        } else {
            PROPS_V(k_props_colour_init, r.dLive, r.dA, r.n);
            rc = props_fixpoint(r, [&] { PROPS_E(k_props_colour_push, r.dFrom, r.dTo, r.m, r.dLive, r.dA, r.dW); });
            if (rc) return rc;
            PROPS_V(k_props_back_init, r.dLive, r.dA, r.dB, r.n);
            rc = props_fixpoint(r, [&] { PROPS_E(k_props_back, r.dFrom, r.dTo, r.m, r.dLive, r.dA, r.dB, r.dW); });
            if (rc) return rc;
            PROPS_V(k_props_colour_apply, r.dLive, r.dB, r.dA, r.dM, r.n, r.dW);
        }
        PRCHK(hipGetLastError());
        PRRC(props_read(r));
        if (r.hW[W_LIVE] <= 0) break;
        rc = props_trim(r);
        if (rc) return rc;
    }
    return SHD_PE_OK;
}

// SHDPE_PROPS_COUNT=plain selects the one-atomic-per-edge counting kernel (the
// measurement of tools/props_time.py); anything else the run-combining one
static bool props_count_runs() {
    const char* e = std::getenv("SHDPE_PROPS_COUNT");
    return !(e && std::strcmp(e, "plain") == 0);
}

static int props_device(PropsRun& r, const ShdPeGraphDesc* g, ShdPeGraphProps* out, int32_t* membership) {
    const int32_t n = r.n;
    const int64_t m = r.m;
    const bool directed = g->directed != 0;
    const size_t nb = (size_t)n;
    PRCHK(hipStreamCreateWithFlags(&r.stream, hipStreamNonBlocking));
    r.stage.stream = r.stream;
    PRCHK(hipEventCreate(&r.ev0));
    PRCHK(hipEventCreate(&r.ev1));
    PRRC(props_alloc(&r.dFrom, (size_t)m));
    PRRC(props_alloc(&r.dTo, (size_t)m));
    PRRC(props_alloc(&r.dCnt, nb));
    PRRC(props_alloc(&r.dM, nb));
    PRRC(props_alloc(&r.dA, nb));
    PRRC(props_alloc(&r.dW, (size_t)W_COUNT));
    PRRC(props_alloc(&r.dSelf, nb));
    if (directed) {
        PRRC(props_alloc(&r.dB, nb));
        PRRC(props_alloc(&r.dLive, nb));
        PRRC(props_alloc(&r.dIn, nb));
        PRRC(props_alloc(&r.dOut, nb));
    }
    if (hipHostMalloc((void**)&r.hW, W_COUNT * sizeof(int32_t)) != hipSuccess) {
        r.hW = nullptr;
        return SHD_PE_ENOMEM;
    }
    r.vGrid = (unsigned)((nb + PROPS_BLOCK - 1) / PROPS_BLOCK);
    r.eGrid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((m + PROPS_BLOCK - 1) / PROPS_BLOCK, PROPS_MAX_GRID));

    PRRC(r.stage.upload(r.dFrom, g->edgeFrom, (size_t)m * 4));
    PRRC(r.stage.upload(r.dTo, g->edgeTo, (size_t)m * 4));
    std::memset(r.hW, 0, W_COUNT * sizeof(int32_t));
    r.hW[W_LIVE] = n;
    r.hW[W_FIRSTINC] = INT_MAX;
    r.hW[W_MINID] = INT_MAX;
    PRCHK(hipMemcpyAsync(r.dW, r.hW, W_COUNT * sizeof(int32_t), hipMemcpyHostToDevice, r.stream));
    PRCHK(hipEventRecord(r.ev0, r.stream));
    PRCHK(hipMemsetAsync(r.dCnt, 0, nb * 4, r.stream));
    PRCHK(hipMemsetAsync(r.dSelf, 0, nb, r.stream));

    // the counting sweep checks every endpoint: nothing else runs on a bad one
    if (r.sweeps >= r.budget) { r.handOff = true; return SHD_PE_OK; }
    ++r.sweeps;
    if (props_count_runs()) PROPS_E(k_props_count<true>, r.dFrom, r.dTo, m, n, (int32_t)directed, r.dCnt, r.dSelf, r.dW);
    else PROPS_E(k_props_count<false>, r.dFrom, r.dTo, m, n, (int32_t)directed, r.dCnt, r.dSelf, r.dW);
    PRCHK(hipGetLastError());
    PRRC(props_read(r));
    if (r.hW[W_ERR]) return SHD_PE_EINVAL;
    PROPS_V(k_props_complete, r.dCnt, r.dSelf, n, r.dW);

    const int rc = directed ? props_directed(r) : props_undirected(r);
    if (rc < 0) return rc;
    if (r.handOff) return SHD_PE_OK;

    // cluster sizes in the counting array (done with it)
    PRCHK(hipMemsetAsync(r.dCnt, 0, nb * 4, r.stream));
    PROPS_V(k_props_sizes, r.dM, r.dCnt, n);
    PROPS_V(k_props_summary, r.dM, r.dCnt, n, r.dW);
    PRCHK(hipGetLastError());
    PRCHK(hipEventRecord(r.ev1, r.stream));
    if (membership) PRCHK(hipMemcpyAsync(membership, r.dM, nb * 4, hipMemcpyDeviceToHost, r.stream));
    PRRC(props_read(r));
    const int32_t first = r.hW[W_FIRSTINC] == INT_MAX ? -1 : r.hW[W_FIRSTINC];
    out->isDirected = directed;
    out->clusterCount = r.hW[W_CLUSTERS];
    out->isConnected = out->clusterCount == 1;
    out->largestCluster = r.hW[W_LARGEST];
    out->isComplete = first < 0;
    out->firstIncomplete = first;
    return SHD_PE_OK;
}

}  // namespace shdpe

using namespace shdpe;

extern "C" int shd_pe_graph_props(const ShdPeGraphDesc* g, int32_t device, int32_t sweepBudget,
                                  ShdPeGraphProps* out, int32_t* membership, ShdPeGraphPropsInfo* info) {
    if (info) std::memset(info, 0, sizeof(*info));
    if (!g || !out || g->nVertices <= 0 || g->nEdges < 0) return SHD_PE_EINVAL;
    if (g->nEdges > 0 && (!g->edgeFrom || !g->edgeTo)) return SHD_PE_EINVAL;
    if (g->nEdges > INT32_MAX / 2) return SHD_PE_ETOOBIG;
    int nDev = 0;
    if (hipGetDeviceCount(&nDev) != hipSuccess || device < 0 || device >= nDev) return SHD_PE_ENODEV;
    if (hipSetDevice(device) != hipSuccess) return SHD_PE_ENODEV;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return SHD_PE_ENODEV;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return SHD_PE_ENODEV;

    const auto t0 = std::chrono::steady_clock::now();
    int rc;
    int64_t usDevice = 0;
    bool handOff;
    int64_t sweeps, rounds;
    {
        PropsRun r;
        r.device = device;
        r.n = g->nVertices;
        r.m = g->nEdges;
        r.budget = sweepBudget > 0 ? sweepBudget : PROPS_DEFAULT_BUDGET;
        rc = props_device(r, g, out, membership);
        handOff = r.handOff;
        sweeps = r.sweeps;
        rounds = r.rounds;
        if (!rc) {
            // a hand-off ends the device part here: its sweeps are what usDevice covers
            if (handOff && (hipEventRecord(r.ev1, r.stream) != hipSuccess ||
                            hipStreamSynchronize(r.stream) != hipSuccess))
                rc = SHD_PE_EHIP;
            float ms = 0.f;
            if (!rc && hipEventElapsedTime(&ms, r.ev0, r.ev1) == hipSuccess) usDevice = (int64_t)(ms * 1000.0f);
        }
    }                                                      // device memory released before a host run
    if (!rc && handOff) rc = shd_pe_graph_props_host(g, out, membership);
    if (info) {
        info->sweeps = sweeps;
        info->rounds = rounds;
        info->handedOff = handOff;
        info->usDevice = usDevice;
        info->usCall =
            std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    }
    return rc;
}
