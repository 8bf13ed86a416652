// pe_aux.hip -- batched per-vertex / per-pair helpers of the path table
// (SURVEY.md §8(f) rank 3): the lookups Shadow otherwise does one at a time
// on the host, with igraph attribute calls per query.
//
//   k_self_paths    _topology_computeShortestPathToSelf  topology.c:1545-1653
//   k_pairs         _topology_lookupDirectPath           topology.c:1877-1927
//                   _topology_verticesAreAdjacent        topology.c:1248-1264
//   k_incident_min  _topology_isComplete                 topology.c:450-552
//
// All are gathers over the CSR (col / lat / rel, rows sorted by neighbour id
// = igraph incidence order): HBM/L2 latency-bound, no arithmetic to speak of.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "pe_device.hpp"
#include "pe_devutil.hpp"
#include "shd_pathengine.h"

namespace shdpe {

// One wave per vertex.  The reference walks v's OUT-incident edges in igraph
// order (ascending neighbour, the self-loop in place) and keeps the first
// strict minimum of the latency (the minLatency == 0 sentinel of :1592 only
// seeds it: latencies are > 0).  That is the lexicographic minimum of
// (latency, incidence position): lanes take strided arcs, then a wave
// reduction.  lat = 2 * w_min, rel = r_min * r_min (:1640-1641).
__global__ __launch_bounds__(256) void k_self_paths(DevGraph g0, const int32_t* __restrict__ verts,
                                                    int32_t count, int64_t nEdges,
                                                    double* __restrict__ lat,
                                                    double* __restrict__ rel,
                                                    uint8_t* __restrict__ flags) {
    const DevGraph g = global_view(g0);
    const int w = (int)(((size_t)blockIdx.x * 256 + threadIdx.x) >> 6);
    const int lane = threadIdx.x & 63;
    if (w >= count) return;                                   // uniform per wave
    const int v = verts[w];
    if (v < 0 || v >= g.n) {
        if (lane == 0) { lat[w] = 0.0; rel[w] = 0.0; flags[w] = F_INVALID; }
        return;
    }
    const int b = g.rowPtr[v], e = g.rowPtr[v + 1];
    const int sp = row_lower_bound(g, v, v) - b;               // self-loop's incidence slot
    const bool self = g.hasSelf[v] != 0;
    double bl = INFINITY, br = 0.0;
    int bp = INT32_MAX;
    for (int a = b + lane; a < e; a += 64) {
        const double L = g.lat[a];
        const int pos = (a - b) + ((self && a - b >= sp) ? 1 : 0);
        if (L < bl || (L == bl && pos < bp)) { bl = L; bp = pos; br = g.srel ? g.srel[a] : g.rel[a]; }
    }
    if (lane == 0 && self) {
        const double L = g.selfMinLat[v];
        if (L < bl || (L == bl && sp < bp)) { bl = L; bp = sp; br = g.selfMinRel[v]; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ol = __shfl_xor(bl, o, 64);
        const double orr = __shfl_xor(br, o, 64);
        const int op = __shfl_xor(bp, o, 64);
        if (ol < bl || (ol == bl && op < bp)) { bl = ol; bp = op; br = orr; }
    }
    if (lane == 0) {
        if (bp == INT32_MAX) {
            // no incident edge: minLatency stays 0 (lat 0, rel 0); the
            // reference errors out only on an edgeless graph
            lat[w] = 0.0;
            rel[w] = 0.0;
            flags[w] = nEdges == 0 ? F_NOEDGE : 0;
        } else {
            lat[w] = 2.0 * bl;
            rel[w] = br * br;
            flags[w] = 0;
        }
    }
}

// _topology_lookupDirectPath over the arc find_arc found: lat = 0.0 + w of the
// newest parallel edge (flat[] where it is not the fastest), rel =
// ((1 * a_s) * a_t) * r_e.  Shared by k_pairs and the prefer-direct pack
// kernel so that the two cannot drift apart.
__device__ __forceinline__ void direct_values(const DevGraph& g, int s, int t, int arc, double* L,
                                              double* R) {
    double acc = 1.0 * g.vrel[s];                            // :1901-1907
    acc = acc * g.vrel[t];
    const double w = s == t ? g.selfLat[s] : (g.flat ? g.flat[arc] : g.lat[arc]);   // get_eid: newest
    const double r = s == t ? g.selfRel[s] : g.rel[arc];
    *L = 0.0 + w;                                            // :1920
    *R = acc * r;                                            // :1921
}

// One thread per pair.  mode 0: direct path (lat = 0.0 + w, rel =
// ((1 * a_s) * a_t) * r_e, flags F_DIRECT or F_NOEDGE); mode 1: adjacency
// only (flags[i] = 1 adjacent, 0 not; s == t adjacent iff it has a loop).
__global__ __launch_bounds__(256) void k_pairs(DevGraph g0, const int32_t* __restrict__ src,
                                               const int32_t* __restrict__ dst, int64_t count,
                                               int mode, double* __restrict__ lat,
                                               double* __restrict__ rel,
                                               uint8_t* __restrict__ flags) {
    const DevGraph g = global_view(g0);
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const int s = src[i], t = dst[i];
    if (s < 0 || s >= g.n || t < 0 || t >= g.n) {
        if (mode == 0) { lat[i] = 0.0; rel[i] = 0.0; }
        flags[i] = mode == 0 ? F_INVALID : 0;
        return;
    }
    int a = -1;
    const bool found = find_arc(g, s, t, &a);
    if (mode == 1) {
        flags[i] = found ? 1 : 0;
        return;
    }
    double L = 0.0, R = 0.0;
    uint8_t f = F_NOEDGE;
    if (found) {
        direct_values(g, s, t, a, &L, &R);
        f = F_DIRECT;
    }
    lat[i] = L;
    rel[i] = R;
    flags[i] = f;
}

// _topology_isComplete: every vertex's incident count (self-loop counted
// twice undirected, then corrected by one) must reach n.  Minimum count.
// Multigraphs pass the host's per-vertex edge counts (merged rows hold one
// arc per neighbour, the reference counts every parallel edge).
__global__ __launch_bounds__(256) void k_incident_min(DevGraph g0, const int32_t* __restrict__ edgeCount,
                                                      int32_t* out) {
    const DevGraph g = global_view(g0);
    const int v = blockIdx.x * 256 + threadIdx.x;
    int c = INT32_MAX;
    if (v < g.n) {
        if (edgeCount) {
            c = edgeCount[v];
        } else {
            c = g.rowPtr[v + 1] - g.rowPtr[v];
            // a loop counts once directed; twice undirected, minus the one
            // correction of :505-519 -- once either way
            if (g.hasSelf[v]) c += 1;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c = min(c, __shfl_xor(c, o, 64));
    if ((threadIdx.x & 63) == 0 && c != INT32_MAX) atomicMin(out, c);
}

void launch_self_paths(const DevGraph& g, const int32_t* dVerts, int32_t count, int64_t nEdges,
                       double* dLat, double* dRel, uint8_t* dFlags, void* stream) {
    if (count <= 0) return;
    const int blocks = (int)(((int64_t)count * 64 + 255) / 256);
    hipLaunchKernelGGL(k_self_paths, dim3(blocks), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), g, dVerts, count, nEdges, dLat,
                       dRel, dFlags);
}

void launch_pairs(const DevGraph& g, const int32_t* dSrc, const int32_t* dDst, int64_t count,
                  int mode, double* dLat, double* dRel, uint8_t* dFlags, void* stream) {
    if (count <= 0) return;
    hipLaunchKernelGGL(k_pairs, dim3((unsigned)((count + 255) / 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), g, dSrc, dDst, count, mode, dLat,
                       dRel, dFlags);
}

void launch_incident_min(const DevGraph& g, const int32_t* dEdgeCount, int32_t* dOut, void* stream) {
    hipLaunchKernelGGL(k_incident_min, dim3((g.n + 255) / 256), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), g, dEdgeCount, dOut);
}

}  // namespace shdpe

namespace shdpe {

// ---------------------------------------------------------------------------
// Row checksums (multi-GPU verification, no reference counterpart): a 64-bit
// fingerprint per table row, the wrapping sum over its entries j and fields f
// of splitmix64(bits(f, j) ^ (j * K + c_f)) -- order-free over j so a
// workgroup reduces it in any order, position-keyed so swapped entries or
// rows change it.  Owners fingerprint their rows before an exchange, every
// rank fingerprints the assembled table after it (bench.py; a numpy twin in
// shdpe/engine.py pins the formula on the CPU).  One 256-thread workgroup per
// row: a coalesced streaming read of the row's 25-29 B per entry.
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
constexpr uint64_t CK_K = 0x9e3779b97f4a7c15ull, CK_C = 0xd1b54a32d192ed03ull;

__global__ __launch_bounds__(256) void k_row_checksums(DevTable tab0, int64_t firstLocal,
                                                       uint64_t* __restrict__ out) {
    const DevTable tab = global_view(tab0);
    __shared__ uint64_t part[4];
    const int64_t T = tab.T;
    const size_t base = (size_t)(firstLocal + blockIdx.x) * (size_t)T;
    uint64_t h = 0;
    for (int64_t j = threadIdx.x; j < T; j += 256) {
        const uint64_t kj = (uint64_t)j * CK_K;
        const size_t o = base + (size_t)j;
        h += mix64((uint64_t)__double_as_longlong(__builtin_nontemporal_load(&tab.lat[o])) ^ (kj + CK_C));
        h += mix64((uint64_t)__double_as_longlong(__builtin_nontemporal_load(&tab.rel[o])) ^ (kj + 2 * CK_C));
        h += mix64((uint64_t)(uint32_t)__builtin_nontemporal_load(&tab.hops[o]) ^ (kj + 3 * CK_C));
        h += mix64((uint64_t)__builtin_nontemporal_load(&tab.flags[o]) ^ (kj + 4 * CK_C));
        if (tab.pred) h += mix64((uint64_t)(uint32_t)__builtin_nontemporal_load(&tab.pred[o]) ^ (kj + 5 * CK_C));
    }
    for (int d = 32; d >= 1; d >>= 1) h += __shfl_xor(h, d, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = h;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

void launch_row_checksums(const DevTable& tab, int64_t firstLocal, int32_t rows, uint64_t* dOut,
                          void* stream) {
    if (rows <= 0) return;
    hipLaunchKernelGGL(k_row_checksums, dim3(rows), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       tab, firstLocal, dOut);
}

}  // namespace shdpe

namespace shdpe {

// ---------------------------------------------------------------------------
// Path-cache image (shd_pe_fill_rowstore[_ex]): the triangular row store of
// pe_rowstore.cpp filled from the whole table exactly as this sequence of
// host calls on an empty store would fill it:
//   1. shd_rowstore_store_rows over rows 0, 1, ..., T-1 in order
//      (topology.c:1805-1864 per row, :1307-1386 per target), with the
//      prefersDirectPaths adjacency when SHD_PE_FILL_PREFER_DIRECT is set;
//   2. with SHD_PE_FILL_DIRECT_PAIRS, shd_rowstore_store(isDirect = 1) of the
//      _topology_lookupDirectPath values (:1877-1927) for every ordered pair
//      (p, q) in position order that topology.c:2019-2021 serves directly
//      (complete graph, or prefersDirectPaths and adjacent).
// One workgroup per triangular row a, three instantiations:
//   PACK_PLAIN     slot (a, a + k) takes row a's entry a + k when that fold
//                  succeeded (neither F_UNREACHABLE nor F_NOEDGE), else row
//                  a + k's entry a (stored under the reversed key), else
//                  stays empty: coalesced along row a, the reverse column
//                  gathered only for the (rare) failed forward entries.
//   PACK_COMPLETE  a complete graph's table (k_direct_rows) with DIRECT_PAIRS:
//                  the same slot rule, the entries ARE the direct paths
//                  (F_NOEDGE where the edge is missing): S_DIRECT is set.
//   PACK_ADJ       prefersDirectPaths (or a complete graph whose table holds
//                  Dijkstra rows, forceMode): per slot, u = attached[a], v =
//                  attached[a + k], the first of
//                    forward fold ok and not (P and u->v)   non-direct
//                    k > 0, reverse fold ok, not (P and v->u)   non-direct, REVERSED
//                    D and P and u->v                       direct
//                    k > 0, D and P and v->u                direct, REVERSED
//                  (a complete graph: P set, the non-direct branches off).
//                  Adjacency comes from two T-bit bitmaps in LDS, Aout (arcs
//                  u -> attached[q]) and Ain (attached[q] -> u; the same
//                  bitmap when undirected), which the workgroup fills first by
//                  striding over u's OUT (and IN) arcs and mapping each head
//                  through posOf[]: one row's arcs are read once, instead of
//                  T binary searches per row.  Only slots of a direct branch
//                  look the arc up (direct_values, k_pairs' arithmetic).
//
// The kernel packs a VIEW of the table (PackView): triangular rows [lo, hi),
// read from a table that holds them at local row a - tab.rowStart, into an
// image segment that starts at off[lo].  The whole table is the view [0, T).
// A row shard (shd_pe_fill_rowstore_shards) is a view whose reverse entry
// (b, a) with b >= hi lies in another shard's rows: wherever the rule above
// would look at it, the slot is a NEED.  It gets what the rule's remaining
// (direct) branches give, plus PACK_S_PENDING in its state byte, stays out of
// the count / minimum accumulators, and is counted in needCount[a - lo] (one
// plain store per workgroup).  The host resolves needs with the two kernels
// below and pe_fill.cpp; no PENDING bit reaches a row store.
//   k_pack_needs   one workgroup per row with needs: its PENDING slots as
//                  (a, b) pairs at the row's prefix offset, in slot order
//                  (wave64 ballot + popcount: no atomics, no scheduling in
//                  the list's content)
//   k_pack_answer  on the owner of row b, one thread per need: ok = the fold
//                  (b, a) succeeded, with its lat / rel
// ---------------------------------------------------------------------------
constexpr int PACK_PLAIN = 0, PACK_COMPLETE = 1, PACK_ADJ = 2;

struct PackNone {};
struct PackAdj {
    DevGraph g;              // caller's ids (the graph posOf / attached index)
    const int32_t* posOf;    // [n] vertex -> table position or -1
    int32_t words;           // 32-bit words per bitmap, (T + 31) / 32
    int32_t direct;          // SHD_PE_FILL_DIRECT_PAIRS
    int32_t complete;        // complete graph: no non-direct entry
};

template <int MODE>
__global__ __launch_bounds__(256) void k_pack_rowstore(
    DevTable tab0, PackView pv, const int64_t* __restrict__ off, uint8_t* __restrict__ img,
    unsigned long long* __restrict__ acc, int32_t* __restrict__ needCount,
    std::conditional_t<MODE == PACK_ADJ, PackAdj, PackNone> pa) {
    const DevTable tab = global_view(tab0);
    __shared__ unsigned long long cnt[4], mnb[4];
    __shared__ int ndc[4];
    const int64_t T = tab.T;
    const int64_t a = pv.lo + blockIdx.x, len = T - a, hi = pv.hi;
    const size_t rowA = (size_t)(a - tab.rowStart) * (size_t)T;   // row a in the view's table
    uint8_t* base = img + (off[a] - off[pv.lo]) + SHD_ROWSTORE_IMAGE_HEADER;
    double* L = reinterpret_cast<double*>(base);
    double* R = L + len;
    uint8_t* S = reinterpret_cast<uint8_t*>(R + len);
    constexpr uint8_t FAILED = F_UNREACHABLE | F_NOEDGE;
    constexpr uint8_t DIRECT = MODE == PACK_COMPLETE ? SHD_ROWSTORE_S_DIRECT : 0;
    unsigned long long c = 0, mn = INF_BITS;
    int nd = 0;                                   // this thread's needs
    if constexpr (MODE == PACK_ADJ) {
        extern __shared__ uint32_t adjBits[];
        const DevGraph g = global_view(pa.g);
        const int32_t* __restrict__ posOf = as_global(pa.posOf);
        const bool directed = g.inCol != g.col;
        uint32_t* Aout = adjBits;
        uint32_t* Ain = directed ? adjBits + pa.words : adjBits;
        for (int w = threadIdx.x; w < (directed ? 2 : 1) * pa.words; w += 256) adjBits[w] = 0u;
        __syncthreads();
        const int u = g.attached[a];
        for (int e = g.rowPtr[u] + threadIdx.x; e < g.rowPtr[u + 1]; e += 256) {
            const int q = posOf[g.col[e]];
            if (q >= 0) atomicOr(&Aout[q >> 5], 1u << (q & 31));
        }
        if (directed)
            for (int e = g.inPtr[u] + threadIdx.x; e < g.inPtr[u + 1]; e += 256) {
                const int q = posOf[g.inCol[e]];
                if (q >= 0) atomicOr(&Ain[q >> 5], 1u << (q & 31));
            }
        if (threadIdx.x == 0 && g.hasSelf[u]) {
            atomicOr(&Aout[a >> 5], 1u << (a & 31));
            if (directed) atomicOr(&Ain[a >> 5], 1u << (a & 31));
        }
        __syncthreads();
        const bool nonDirect = !pa.complete, wantDirect = pa.direct != 0;
        for (int64_t k = threadIdx.x; k < len; k += 256) {
            const int64_t b = a + k;
            const size_t fo = rowA + b;
            const size_t ro = (size_t)(b - tab.rowStart) * T + a;  // (read only where b < hi)
            const bool adjF = (Aout[b >> 5] >> (b & 31)) & 1u;     // u -> v
            const bool adjR = (Ain[b >> 5] >> (b & 31)) & 1u;      // v -> u
            double lat = 0.0, rel = 0.0;
            uint8_t s = 0;
            const bool wantRev = nonDirect && k > 0 && !adjR;     // the rule may look at entry (b, a)
            bool need = false;
            if (nonDirect && !adjF && !(tab.flags[fo] & FAILED)) {
                lat = tab.lat[fo];
                rel = tab.rel[fo];
                s = SHD_ROWSTORE_S_STORED;
            } else if (wantRev && b < hi && !(tab.flags[ro] & FAILED)) {
                lat = tab.lat[ro];
                rel = tab.rel[ro];
                s = SHD_ROWSTORE_S_STORED | SHD_ROWSTORE_S_REVERSED;
            } else {
                need = wantRev && b >= hi;             // row b is behind the view: the direct entry meanwhile
                if (wantDirect && (adjF || (k > 0 && adjR))) {
                    const int v = g.attached[b];
                    const int from = adjF ? u : v, to = adjF ? v : u;
                    int arc = -1;
                    if (find_arc(g, from, to, &arc)) {     // (always: the bitmaps came from these arcs)
                        direct_values(g, from, to, arc, &lat, &rel);
                        s = SHD_ROWSTORE_S_STORED | SHD_ROWSTORE_S_DIRECT |
                            (adjF ? 0 : SHD_ROWSTORE_S_REVERSED);
                    }
                }
            }
            L[k] = lat;
            R[k] = rel;
            S[k] = need ? (uint8_t)(s | PACK_S_PENDING) : s;
            if (need) {
                ++nd;
            } else if (s) {
                ++c;
                const unsigned long long lb = (unsigned long long)__double_as_longlong(lat);
                mn = lb < mn ? lb : mn;
            }
        }
    } else {
        for (int64_t k = threadIdx.x; k < len; k += 256) {
            const int64_t b = a + k;
            const size_t fo = rowA + b;
            double lat = 0.0, rel = 0.0;
            uint8_t s = 0;
            if (!(tab.flags[fo] & FAILED)) {
                lat = tab.lat[fo];
                rel = tab.rel[fo];
                s = SHD_ROWSTORE_S_STORED | DIRECT;
            } else if (k > 0) {
                if (b >= hi) {                   // a need: empty until answered
                    s = PACK_S_PENDING;
                    ++nd;
                } else {
                    const size_t ro = (size_t)(b - tab.rowStart) * T + a;
                    if (!(tab.flags[ro] & FAILED)) {
                        lat = tab.lat[ro];
                        rel = tab.rel[ro];
                        s = SHD_ROWSTORE_S_STORED | SHD_ROWSTORE_S_REVERSED | DIRECT;
                    }
                }
            }
            L[k] = lat;
            R[k] = rel;
            S[k] = s;
            if (s & SHD_ROWSTORE_S_STORED) {
                ++c;
                const unsigned long long lb = (unsigned long long)__double_as_longlong(lat);
                mn = lb < mn ? lb : mn;      // stored latencies are > 0: bit order = value order
            }
        }
    }
    for (int d = 32; d >= 1; d >>= 1) {
        c += __shfl_xor(c, d, 64);
        nd += __shfl_xor(nd, d, 64);
        const unsigned long long o = __shfl_xor(mn, d, 64);
        mn = o < mn ? o : mn;
    }
    if ((threadIdx.x & 63) == 0) { cnt[threadIdx.x >> 6] = c; mnb[threadIdx.x >> 6] = mn; ndc[threadIdx.x >> 6] = nd; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long cc = 0, m = INF_BITS;
        for (int w = 0; w < 4; ++w) { cc += cnt[w]; m = mnb[w] < m ? mnb[w] : m; }
        if (cc) atomicAdd(&acc[0], cc);
        if (m != INF_BITS) atomicMin(&acc[1], m);
        if (needCount) needCount[blockIdx.x] = ndc[0] + ndc[1] + ndc[2] + ndc[3];
    }
}

// The needs of image row rows[blockIdx.x] of the view (segment `img` from
// off[pv.lo]) as (a, b) pairs at pairs[2 * pre[blockIdx.x] ...], ascending b:
// its slots k >= hi - a with PACK_S_PENDING, which k_pack_rowstore left there
// by the need rule.  Chunks of 256 slots; per chunk every wave ballots its 64
// slots, the four popcounts give each wave its place, the lanes below a lane
// its place in the wave.
__global__ __launch_bounds__(256) void k_pack_needs(PackView pv, int64_t T, const int64_t* __restrict__ off,
                                                    const uint8_t* __restrict__ img,
                                                    const int32_t* __restrict__ rows,
                                                    const int64_t* __restrict__ pre,
                                                    int32_t* __restrict__ pairs) {
    __shared__ int wc[4];
    const int64_t a = rows[blockIdx.x], len = T - a;
    const uint8_t* S = img + (off[a] - off[pv.lo]) + SHD_ROWSTORE_IMAGE_HEADER + (size_t)len * 16;
    int32_t* out = pairs + 2 * pre[blockIdx.x];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int64_t done = 0;                            // needs written so far (uniform)
    for (int64_t k0 = pv.hi - a; k0 < len; k0 += 256) {      // (hi > a: b >= hi means k >= hi - a >= 1)
        const int64_t k = k0 + threadIdx.x;
        const bool p = k < len && (S[k] & PACK_S_PENDING);
        const unsigned long long m = __ballot(p);
        if (lane == 0) wc[w] = __popcll(m);
        __syncthreads();
        int before = 0, all = 0;
        for (int i = 0; i < 4; ++i) { before += i < w ? wc[i] : 0; all += wc[i]; }
        if (p) {
            const int64_t at = done + before + __popcll(m & ((1ull << lane) - 1ull));
            out[2 * at] = (int32_t)a;
            out[2 * at + 1] = (int32_t)(a + k);
        }
        done += all;
        __syncthreads();                         // wc is rewritten by the next chunk
    }
}

// One thread per need (a, b) of a list whose rows b this table view owns.
__global__ __launch_bounds__(256) void k_pack_answer(DevTable tab0, const int32_t* __restrict__ pairs,
                                                     int64_t n, uint8_t* __restrict__ ok,
                                                     double* __restrict__ lat, double* __restrict__ rel) {
    const DevTable tab = global_view(tab0);
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t a = pairs[2 * i], b = pairs[2 * i + 1];
    const size_t ro = (size_t)(b - tab.rowStart) * (size_t)tab.T + (size_t)a;
    ok[i] = (tab.flags[ro] & (F_UNREACHABLE | F_NOEDGE)) ? 0 : 1;
    lat[i] = tab.lat[ro];
    rel[i] = tab.rel[ro];
}

// per source row: 1 when no target's fold failed (F_NOEDGE; unreachable
// targets do not count), topology.c:1815-1859's isAllSuccess
// (out[i]: the table's local row i)
__global__ __launch_bounds__(256) void k_rows_all_success(DevTable tab0, int32_t* __restrict__ out) {
    const DevTable tab = global_view(tab0);
    __shared__ int bad;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * (size_t)tab.T;
    int b = 0;
    for (int64_t j = threadIdx.x; j < tab.T; j += 256) b |= (tab.flags[base + j] & F_NOEDGE) != 0;
    if (b) bad = 1;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = bad ? 0 : 1;
}

int pack_adj_lds_bytes(int64_t T, bool directed) {
    const int64_t b = (T + 31) / 32 * 4 * (directed ? 2 : 1);
    return b <= 64 * 1024 ? (int)b : -1;
}

int launch_pack_rowstore(const DevTable& tab, const PackView& pv, const int64_t* dOff, uint8_t* dImg,
                         unsigned long long* dAcc, int32_t* dNeedCount, int mode, const DevGraph* g,
                         const int32_t* dPosOf, bool direct, bool complete, void* stream) {
    if (pv.hi <= pv.lo) return 0;
    const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(pv.hi - pv.lo)), block(256);
    if (mode == PACK_ADJ) {
        if (!g || !dPosOf) return -1;
        const int lds = pack_adj_lds_bytes(tab.T, g->inCol != g->col);
        if (lds < 0) return -1;
        const PackAdj pa{*g, dPosOf, (int32_t)((tab.T + 31) / 32), direct ? 1 : 0, complete ? 1 : 0};
        hipLaunchKernelGGL(k_pack_rowstore<PACK_ADJ>, grid, block, (size_t)lds, st, tab, pv, dOff, dImg, dAcc,
                           dNeedCount, pa);
    } else if (mode == PACK_COMPLETE) {
        hipLaunchKernelGGL(k_pack_rowstore<PACK_COMPLETE>, grid, block, 0, st, tab, pv, dOff, dImg, dAcc,
                           dNeedCount, PackNone{});
    } else {
        hipLaunchKernelGGL(k_pack_rowstore<PACK_PLAIN>, grid, block, 0, st, tab, pv, dOff, dImg, dAcc,
                           dNeedCount, PackNone{});
    }
    return 0;
}

void launch_pack_needs(const PackView& pv, int64_t T, const int64_t* dOff, const uint8_t* dImg,
                       const int32_t* dRows, const int64_t* dPre, int32_t nRows, int32_t* dPairs,
                       void* stream) {
    if (nRows <= 0) return;
    hipLaunchKernelGGL(k_pack_needs, dim3((unsigned)nRows), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       pv, T, dOff, dImg, dRows, dPre, dPairs);
}

void launch_pack_answer(const DevTable& tab, const int32_t* dPairs, int64_t n, uint8_t* dOk, double* dLat,
                        double* dRel, void* stream) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_pack_answer, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), tab, dPairs, n, dOk, dLat, dRel);
}

void launch_rows_all_success(const DevTable& tab, int32_t rows, int32_t* dOut, void* stream) {
    if (tab.T <= 0 || rows <= 0) return;
    hipLaunchKernelGGL(k_rows_all_success, dim3((unsigned)rows), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), tab, dOut);
}

}  // namespace shdpe

namespace shdpe {

// ---------------------------------------------------------------------------
// Batched path extraction (shd_pe_get_paths): the igraph paths behind many
// table entries in one call, topology.c:1449 / :1502-1503 / :1831-1841 for
// every (src, dst) of a batch instead of one shd_pe_get_path each.
//
//   k_paths_size   per request: validity, attachment, owner and the table's
//                  flags / hops -> path length and SHD_PE_E* status
//   k_paths_scan   exclusive scan of the lengths -> output offsets
//   k_paths_flags  saves / restores the flag bytes of the rows an emulation
//                  group rewrites (the emulation marks every entry F_EXACT)
//   k_paths_walk   per request: len - 1 parent steps from dst, each vertex
//                  written straight to its final place; arrival at src checked
//   k_paths_hops   per output entry: the hop's edge (igraph_get_eid: the
//                  newest parallel edge) -> latency and 1 - packetloss
//   k_paths_load   (shd_pe_path_load) per output entry: its request's weight
//                  added to the entry's vertex and to the arc into it
//
// The walk is a chain of dependent 4-B loads (parent arc, then its tail), so
// one thread serves one request and the parallelism is across requests; the
// host orders a launch's requests by source, so neighbouring lanes read the
// same parent array.  The hop attributes have no such chain: one thread per
// output entry, coalesced stores.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_paths_size(DevGraph g0, DevTable tab0, PathsSizeArgs p) {
    const DevGraph g = global_view(g0);
    const DevTable tab = global_view(tab0);
    const int32_t* __restrict__ posOf = as_global(p.posOf);
    const int32_t i = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (i >= p.count) return;
    int32_t* __restrict__ len = as_global(p.len);
    int32_t* __restrict__ stat = as_global(p.stat);
    const int s = as_global(p.src)[i], t = as_global(p.dst)[i];
    // outcomes that need no table row: decided by the primary shard
    int st = SHD_PE_OK, L = 0;
    bool table = false;
    int ps = -1, pt = -1;
    if (s < 0 || s >= g.n || t < 0 || t >= g.n) {
        st = SHD_PE_EINVAL;
    } else if ((ps = posOf[s]) < 0 || (pt = posOf[t]) < 0) {
        st = SHD_PE_ENOTATTACHED;
    } else if (s == t) {
        L = 1;                                   // the 1-vertex igraph path [s]
    } else if (p.complete) {                     // _topology_lookupDirectPath: the edge itself
        int a = -1;
        if (find_arc(g, s, t, &a)) L = 2;
        else st = SHD_PE_ENOEDGE;
    } else if (ps < p.ownLo || ps >= p.ownHi) {
        st = SHD_PE_ENOTOWNED;
    } else {
        table = true;
    }
    if (!table) {
        if (p.primary) { len[i] = L; stat[i] = st; }
        return;
    }
    if (ps < p.rowLo || ps >= p.rowHi) return;   // another shard's row: that shard answers
    const size_t cell = (size_t)(ps - tab.rowStart) * (size_t)tab.T + (size_t)pt;
    const uint8_t f = tab.flags[cell];
    if (f & F_UNREACHABLE) st = SHD_PE_EUNREACHABLE;
    else if (f & F_NOEDGE) st = SHD_PE_ENOEDGE;
    else {
        const int h = tab.hops[cell];
        if (h >= 1 && h < g.n) L = h + 1;
        else st = SHD_PE_EHIP;                   // (not a table this engine wrote)
    }
    len[i] = L;
    stat[i] = st;
}

// One workgroup: off[i] = sum of len[0 .. i), off[count] = the total.
__global__ __launch_bounds__(1024) void k_paths_scan(const int32_t* __restrict__ len, int32_t count,
                                                     int64_t* __restrict__ off) {
    __shared__ long long wsum[16];
    __shared__ long long carry;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int32_t base = 0; base < count; base += 1024) {
        const int32_t i = base + tid;
        const long long v = i < count ? (long long)len[i] : 0;
        long long x = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long y = __shfl_up(x, o, 64);
            if (lane >= o) x += y;
        }
        if (lane == 63) wsum[w] = x;
        __syncthreads();
        long long pre = carry;
        for (int k = 0; k < w; ++k) pre += wsum[k];
        if (i < count) off[i] = pre + x - v;
        __syncthreads();
        if (tid == 1023) carry = pre + x;
        __syncthreads();
    }
    if (tid == 0) off[count] = carry;
}

// One workgroup per row: the row's T flag bytes to buf (restore == 0) or back.
__global__ __launch_bounds__(256) void k_paths_flags(DevTable tab0, const int32_t* __restrict__ rows,
                                                     uint8_t* __restrict__ buf, int restore) {
    const DevTable tab = global_view(tab0);
    const int64_t T = tab.T;
    uint8_t* row = tab.flags + (size_t)(rows[blockIdx.x] - tab.rowStart) * (size_t)T;
    uint8_t* sav = buf + (size_t)blockIdx.x * (size_t)T;
    for (int64_t j = threadIdx.x; j < T; j += 256) {
        if (restore) row[j] = sav[j];
        else sav[j] = row[j];
    }
}

__global__ __launch_bounds__(256) void k_paths_walk(DevGraph g0, PathsWalkArgs p) {
    const DevGraph g = global_view(g0);
    const int32_t j = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (j >= p.nReqs) return;
    const PathReq q = as_global(p.reqs)[j];
    const int32_t L = as_global(p.len)[q.req];
    int32_t* __restrict__ out = as_global(p.verts) + as_global(p.off)[q.req];
    if (L <= 0) return;
    if (q.slot < 0) {                            // [s] or, complete graph, [s, t]: caller's ids
        out[0] = q.s;
        if (L > 1) out[1] = q.t;
        return;
    }
    const int32_t* __restrict__ P = as_global(p.parents) + (size_t)q.slot * (size_t)p.stride;
    int v = q.t;
    bool ok = true;
    for (int32_t k = L - 1; k >= 1; --k) {
        out[k] = g.oldId ? g.oldId[v] : v;
        const int a = P[v];
        if (a < 0 || (a & ~TIE_AMB) >= p.nInArcs) { ok = false; break; }
        v = g.inCol[a & ~TIE_AMB];
        if (v < 0 || v >= g.n) { ok = false; break; }
    }
    if (ok && v == q.s) {
        out[0] = g.oldId ? g.oldId[v] : v;
    } else {                                     // not this source's parents: never reported as a path
        as_global(p.failed)[q.req] = 1;
        atomicAdd(as_global(p.nFailed), 1);
    }
}

// The request whose path holds output entry e (0 <= e < off[count]): the last i
// with off[i] <= e.  Empty paths share their successor's offset and are never
// chosen.
__device__ __forceinline__ int32_t entry_request(const int64_t* __restrict__ off, int32_t count, int64_t e) {
    int32_t lo = 0, hi = count;
    while (hi - lo > 1) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= e) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_paths_hops(DevGraph g0, const int64_t* __restrict__ off,
                                                    int32_t count, const int32_t* __restrict__ verts,
                                                    double* __restrict__ hopLat,
                                                    double* __restrict__ hopRel,
                                                    int32_t* __restrict__ nFailed) {
    const DevGraph g = global_view(g0);
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= off[count]) return;
    const int32_t lo = entry_request(off, count, e);
    double L = 0.0, R = 0.0;
    if (e > off[lo]) {
        const int u = verts[e - 1], v = verts[e];
        int a = -1;
        if (u >= 0 && u < g.n && v >= 0 && v < g.n && u != v && find_arc(g, u, v, &a)) {
            L = g.flat ? g.flat[a] : g.lat[a];   // igraph_get_eid: the newest parallel edge
            R = g.rel[a];
        } else {
            atomicAdd(nFailed, 1);
        }
    }
    if (hopLat) hopLat[e] = L;
    if (hopRel) hopRel[e] = R;
}

// shd_pe_path_load's reduction, in k_paths_hops' place: per output entry e the
// weight of its request is added to the entry's vertex (acc[nArcs + v]) and,
// past a path's first entry, to the arc verts[e-1] -> verts[e] (acc[arc], the
// arc k_paths_hops reads its attributes from).  The sums are integers mod 2^64,
// so their order does not matter.  load_entry finds both places; `add` adds.
template <class Add>
__device__ __forceinline__ void load_entry(const DevGraph& g, const int64_t* __restrict__ off, int32_t count,
                                           const int32_t* __restrict__ verts,
                                           const unsigned long long* __restrict__ weight, int64_t nArcs, int64_t e,
                                           int32_t* __restrict__ nFailed, Add add) {
    const int32_t lo = entry_request(off, count, e);
    const unsigned long long w = weight[lo];
    const int v = verts[e];
    if (v < 0 || v >= g.n) {                     // (never a path's vertex: the walks write ids of the graph)
        atomicAdd(nFailed, 1);
        return;
    }
    if (w) add((unsigned long long)(nArcs + v), w);
    if (e > off[lo]) {
        const int u = verts[e - 1];
        int a = -1;
        if (u >= 0 && u < g.n && u != v && find_arc(g, u, v, &a)) {
            if (w) add((unsigned long long)a, w);
        } else {
            atomicAdd(nFailed, 1);
        }
    }
}

// A workgroup takes LOAD_PER_THREAD * 256 consecutive entries (requests sorted
// by source: a few sources' paths, which share the arcs next to them and the
// hubs) and sums them in an LDS table of (place in acc, 64-bit sum) first --
// LDS compare-and-swap on the key, LDS 64-bit add, LOAD_PROBES linear probes,
// then a global no-return 64-bit device-scope add -- and issues one global add
// per occupied slot at the end.  `slots` is a power of two <= LOAD_SLOTS_MAX.
// nIssued (debug counters, else null): the global adds issued.
constexpr int LOAD_SLOTS_MAX = 2048;             // 24 KiB of LDS
constexpr int LOAD_PER_THREAD = 8;
constexpr int LOAD_PROBES = 4;
constexpr uint32_t LOAD_EMPTY = 0xFFFFFFFFu;     // (nArcs + n <= 2^32 - 2: both are int32 counts)

__global__ __launch_bounds__(256) void k_paths_load(DevGraph g0, const int64_t* __restrict__ off,
                                                    int32_t count, const int32_t* __restrict__ verts,
                                                    const unsigned long long* __restrict__ weight,
                                                    int64_t nArcs, unsigned long long* __restrict__ acc,
                                                    int32_t* __restrict__ nFailed, int slots,
                                                    unsigned long long* __restrict__ nIssued) {
    __shared__ uint32_t keys[LOAD_SLOTS_MAX];
    __shared__ unsigned long long sums[LOAD_SLOTS_MAX];
    __shared__ unsigned int issuedWg;
    const DevGraph g = global_view(g0);
    const int tid = threadIdx.x;
    for (int i = tid; i < slots; i += 256) {
        keys[i] = LOAD_EMPTY;
        sums[i] = 0;
    }
    if (tid == 0) issuedWg = 0;
    __syncthreads();
    const uint32_t mask = (uint32_t)slots - 1;
    const int64_t total = off[count];
    const int64_t base = (int64_t)blockIdx.x * (256 * LOAD_PER_THREAD);
    unsigned issued = 0;
    const auto add = [&](unsigned long long at, unsigned long long w) {
        const uint32_t key = (uint32_t)at;
        uint32_t h = ((key * 0x9E3779B1u) >> 11) & mask;
        for (int p = 0; p < LOAD_PROBES; ++p) {
            const uint32_t was = atomicCAS(&keys[h], LOAD_EMPTY, key);
            if (was == LOAD_EMPTY || was == key) {
                atomicAdd(&sums[h], w);
                return;
            }
            h = (h + 1) & mask;
        }
        __hip_atomic_fetch_add(acc + at, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ++issued;
    };
    for (int it = 0; it < LOAD_PER_THREAD; ++it) {
        const int64_t e = base + it * 256 + tid;
        if (e >= total) break;                   // (the barrier below is outside the loop)
        load_entry(g, off, count, verts, weight, nArcs, e, nFailed, add);
    }
    __syncthreads();
    for (int i = tid; i < slots; i += 256) {
        const uint32_t key = keys[i];
        const unsigned long long sum = sums[i];
        if (key != LOAD_EMPTY && sum) {
            __hip_atomic_fetch_add(acc + key, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            ++issued;
        }
    }
    if (nIssued) {                               // (uniform)
        if (issued) atomicAdd(&issuedWg, issued);
        __syncthreads();
        if (tid == 0 && issuedWg) atomicAdd(nIssued, (unsigned long long)issuedWg);
    }
}

// shd_pe_table_load on a complete graph: the path of (attached[p], attached[q])
// is the edge itself, by shd_pe_get_paths' status rule (k_paths_size: [s] for
// p == q, SHD_PE_ENOEDGE where the edge is missing).  blockIdx.y = the row of
// the block, one thread per destination; the row's own vertex and the totals
// are summed in LDS first, one global add each per workgroup.
__global__ __launch_bounds__(256) void k_table_direct(DevGraph g0, TableDirectArgs p) {
    __shared__ unsigned long long part[5];       // totals[0..3], the source's vertex load
    const DevGraph g = global_view(g0);
    const int tid = threadIdx.x;
    if (tid < 5) part[tid] = 0;
    __syncthreads();
    const int r = blockIdx.y, q = (int)(blockIdx.x * 256 + tid);
    const int32_t* __restrict__ att = as_global(p.attached);
    unsigned long long* __restrict__ acc = (unsigned long long*)as_global(p.acc);
    const int s = att[p.row0 + r];
    if (q < p.T) {
        const int t = att[q];
        const unsigned long long w = p.weight ? (unsigned long long)as_global(p.weight)[(size_t)r * (size_t)p.T + q] : 1ull;
        int a = -1;
        if (s == t) {
            atomicAdd(&part[0], 1ull);
            atomicAdd(&part[1], w);
            atomicAdd(&part[4], w);
        } else if (find_arc(g, s, t, &a)) {
            atomicAdd(&part[0], 1ull);
            atomicAdd(&part[1], 2 * w);
            atomicAdd(&part[2], w);
            atomicAdd(&part[4], w);
            if (w) {
                __hip_atomic_fetch_add(acc + a, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_add(acc + p.nArcs + t, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        } else {
            atomicAdd(&part[3], 1ull);
        }
    }
    __syncthreads();
    if (tid < 4 && part[tid])
        __hip_atomic_fetch_add((unsigned long long*)as_global(p.out) + tid, part[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid == 4 && part[4])
        __hip_atomic_fetch_add(acc + p.nArcs + s, part[4], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

void launch_table_direct(const DevGraph& gAux, const TableDirectArgs& a, void* stream) {
    if (a.rows <= 0 || a.T <= 0) return;
    hipLaunchKernelGGL(k_table_direct, dim3((unsigned)((a.T + 255) / 256), (unsigned)a.rows), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), gAux, a);
}

// k_tree_load_parents (shd_pe_table_load's parent tier, launch_tree_load_parents):
// k_tree_load's reduction for sources whose parents stand in an explicit array
// of in-arc words, read by k_paths_walk's rule -- the scratch slots of
// k_sparse_rows' row-less form, or the tie slots after the early-stop emulation
// -- or of vertex ids: the parent rows the dense predecessor pass leaves
// (PAR_VERTEX below).
//
// Persistent workgroups, one listed source at a time, each with a private
// scratch slot of (sum, pending children, claimed mark) per vertex that it
// reuses for its next source.  Per source, with a workgroup barrier between
// the steps:
//   init    the slot cleared.  A source with a skip byte does not run at all; one
//           whose tie slot's threshold is NaN (the emulation's consistency check
//           failed it) is handed on
//   seed    per destination: status and hops from the table row -> the totals
//           and the expected sum; a status-0 destination of non-zero weight adds
//           its weight to its vertex and
//   claim   walks up from it, marking each vertex once (compare-and-swap) and
//           counting it as a child of its parent, until the source or a marked
//           vertex.  A parent word that is negative, names no in-arc, or whose
//           tail is no vertex fails the source.  A cycle ends on the marks
//   sum     as k_tree_load: who takes an entry without pending children adds
//           its sum to the parent's and, after the last child, goes on with it
//   check   the source passes when it did not fail, (A) the sum at its vertex is
//           the expected one and (B) the sums of all claimed vertices add up to
//           the table's weighted vertex count (tot[1]): the chains are as long
//           as the table's hops say (k_paths_walk's check through L).  A cycle
//           is never summed and fails (A)
//   commit  per claimed vertex its sum to the vertex's place in acc and to the
//           place of the arc from its parent (caller's ids, find_arc; over vertex
//           ids a full out-row's arc at its computed place first), with
//           device-scope no-return adds.  (Per-workgroup accumulators flushed
//           once per launch were measured and were slower: DESIGN §8h.)
// Nothing reaches acc or the totals before the check.  Every loop ends on
// a mark, a count or a bound; the slot's traffic is workgroup scope.
constexpr int TPAR_THREADS = 512;

__device__ __forceinline__ void wg_add(unsigned long long* p, unsigned long long v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void dev_add(unsigned long long* p, unsigned long long v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// How a source's parents stand in its array (the kernel's compile-time parameter):
// PAR_INARC   in-arc words, as k_paths_walk reads them (TIE_AMB masked off)
// PAR_VERTEX  the parent's vertex id in g's ids -- the rows the dense predecessor
//             pass leaves (k_minplus<MP_PRED>: -1 none, -2 a tie, else the vertex)
// tpar_parent: the checked read of the claim step, -1 = the word is refused (it
// is negative, names no in-arc, its tail is no vertex; a vertex id out of
// [0, n) or the vertex itself).  tpar_tail: the same parent once claimed.
enum { PAR_INARC = 0, PAR_VERTEX = 1 };

template <int PAR>
__device__ __forceinline__ int tpar_parent(const DevGraph& g, const int32_t* __restrict__ P, int x, int n,
                                           int nInArcs) {
    if constexpr (PAR == PAR_VERTEX) {
        const int u = P[x];
        return (u < 0 || u >= n || u == x) ? -1 : u;
    } else {
        const int a = P[x];
        if (a < 0 || (a & ~TIE_AMB) >= nInArcs) return -1;
        const int u = g.inCol[a & ~TIE_AMB];
        return (u < 0 || u >= n) ? -1 : u;
    }
}
template <int PAR>
__device__ __forceinline__ int tpar_tail(const DevGraph& g, const int32_t* __restrict__ P, int x) {
    if constexpr (PAR == PAR_VERTEX) return P[x];
    else return g.inCol[P[x] & ~TIE_AMB];
}

template <int PAR>
__global__ __launch_bounds__(TPAR_THREADS) void k_tree_load_parents(DevGraph g0, DevGraph aux0, DevTable tab0,
                                                                    TreeParentsArgs p) {
    __shared__ unsigned long long expect, tot[3], total, claimedSrc, issuedWg, claimedWg;
    __shared__ unsigned int bad;
    __shared__ int run, fail, pass;
    const DevGraph g = global_view(g0);
    const DevGraph aux = global_view(aux0);
    const DevTable tab = global_view(tab0);
    const int tid = threadIdx.x, n = g.n;
    const int64_t T = tab.T;
    unsigned long long* __restrict__ sum = (unsigned long long*)as_global(p.sum) + (size_t)blockIdx.x * (size_t)n;
    int32_t* __restrict__ pend = as_global(p.pend) + (size_t)blockIdx.x * (size_t)n;
    int32_t* __restrict__ mark = as_global(p.mark) + (size_t)blockIdx.x * (size_t)n;
    const int32_t* __restrict__ attDev = as_global(p.attDev);
    unsigned long long* __restrict__ acc = (unsigned long long*)as_global(p.acc);
    unsigned long long* __restrict__ out = (unsigned long long*)as_global(p.out);
    if (tid == 0) issuedWg = claimedWg = 0;
    for (int i = blockIdx.x; i < p.nSrc; i += gridDim.x) {
        const int pos = as_global(p.pos)[i];
        const int slot = p.slot ? as_global(p.slot)[i] : i;
        const int src = attDev[pos];
        const int32_t* __restrict__ P = as_global(p.parents) + (size_t)slot * (size_t)p.stride;
        const unsigned long long* __restrict__ W =
            p.weight ? (const unsigned long long*)as_global(p.weight) + (size_t)i * (size_t)T : nullptr;
        const bool target = i == p.corruptAt;
        // ---- init
        if (tid == 0) {
            run = !(p.skip && as_global(p.skip)[i] != 0);
            const double thr = p.thr ? as_global(p.thr)[slot] : 0.0;
            fail = thr != thr;
            pass = 0;
            expect = tot[0] = tot[1] = tot[2] = total = claimedSrc = 0;
            bad = 0;
        }
        for (int v = tid; v < n; v += TPAR_THREADS) {
            sum[v] = 0;
            pend[v] = 0;
            mark[v] = 0;
        }
        fence_wg();
        __syncthreads();
        const bool runs = run != 0, sound = fail == 0;   // (the same in every thread)
        if (!runs) {
            __syncthreads();                     // (read before the next source's init writes it)
            continue;
        }
        // ---- seed and claim
        for (int q = tid; q < T && sound; q += TPAR_THREADS) {
            unsigned long long hops = 0;
            if (q != pos) {
                const size_t cell = (size_t)(pos - tab.rowStart) * (size_t)T + (size_t)q;
                if (tab.flags[cell] & (F_UNREACHABLE | F_NOEDGE)) {
                    atomicAdd(&bad, 1u);
                    continue;
                }
                const int h = tab.hops[cell];
                if (h < 1 || h >= n) {           // (not a table this engine wrote: the request route says so)
                    fail = 1;
                    continue;
                }
                hops = (unsigned long long)h;
            }
            const unsigned long long w = W ? W[q] : 1ull;
            atomicAdd(&tot[0], 1ull);
            if (w == 0) continue;                // adds nothing anywhere
            atomicAdd(&tot[1], w * (hops + 1));
            atomicAdd(&tot[2], w * hops);
            atomicAdd(&expect, w);
            int x = attDev[q];
            wg_add(&sum[x], w);
            while (!*(volatile int*)&fail) {
                int32_t was = 0;
                if (!__hip_atomic_compare_exchange_strong(&mark[x], &was, 1, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                          __HIP_MEMORY_SCOPE_WORKGROUP))
                    break;                       // claimed already: the rest of the way is too
                if (x == src) break;
                const int u = tpar_parent<PAR>(g, P, x, n, p.nInArcs);
                if (u < 0 || (target && p.corrupt == 2)) {
                    fail = 1;
                    break;
                }
                __hip_atomic_fetch_add(&pend[u], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                x = u;                           // (every step claims a vertex: at most n of them)
            }
        }
        fence_wg();
        __syncthreads();
        // ---- sum, leaves first (every claimed vertex but the source has a checked parent)
        const bool whole = fail == 0;
        for (int v = tid; v < n && whole; v += TPAR_THREADS) {
            if (!ld_wg(&mark[v])) continue;
            int e = v;
            for (;;) {
                int32_t zero = 0;
                if (!__hip_atomic_compare_exchange_strong(&pend[e], &zero, -1, __ATOMIC_ACQUIRE, __ATOMIC_RELAXED,
                                                          __HIP_MEMORY_SCOPE_WORKGROUP))
                    break;                       // children pending, or taken by another thread
                if (e == src) break;             // its sum stays for the check
                // (the entry's sum is final: every child added before it counted down)
                const unsigned long long s = __hip_atomic_fetch_add(&sum[e], 0ull, __ATOMIC_RELAXED,
                                                                    __HIP_MEMORY_SCOPE_WORKGROUP);
                const int u = tpar_tail<PAR>(g, P, e);
                wg_add(&sum[u], s);
                if (__hip_atomic_fetch_sub(&pend[u], 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP) != 1) break;
                e = u;
            }
        }
        fence_wg();
        __syncthreads();
        // ---- check
        {
            unsigned long long part = 0, cl = 0;
            for (int v = tid; v < n && whole; v += TPAR_THREADS)
                if (ld_wg(&mark[v])) {
                    ++cl;
                    part += ld_wg(&sum[v]);
                }
            if (cl) {
                atomicAdd(&total, part);
                atomicAdd(&claimedSrc, cl);
            }
        }
        __syncthreads();
        if (tid == 0) {
            const unsigned long long wantA = expect + (target && p.corrupt == 1 ? 1ull : 0ull);
            const unsigned long long wantB = tot[1] + (target && p.corrupt == 3 ? 1ull : 0ull);
            const bool ok = whole && ld_wg(&sum[src]) == wantA && total == wantB;
            pass = ok;
            as_global(p.handed)[i] = ok ? 0 : 1;
            if (ok) {
                dev_add(&out[0], tot[0]);
                dev_add(&out[1], tot[1]);
                dev_add(&out[2], tot[2]);
                dev_add(&out[3], (unsigned long long)bad);
                dev_add(&out[4], 1ull);
                claimedWg += claimedSrc;
            }
        }
        __syncthreads();
        // ---- commit
        unsigned long long issued = 0;
        for (int v = tid; v < n && pass; v += TPAR_THREADS) {
            if (!ld_wg(&mark[v])) continue;
            const unsigned long long s = ld_wg(&sum[v]);
            if (s == 0) continue;
            const int ov = g.oldId ? g.oldId[v] : v;
            dev_add(acc + p.nArcs + ov, s);
            ++issued;
            if (v == src) continue;
            const int u = tpar_tail<PAR>(g, P, v);
            const int ou = g.oldId ? g.oldId[u] : u;
            int arc = -1;
            bool found = false;
            if constexpr (PAR == PAR_VERTEX) {
                // a full out-row (every other vertex, ascending) holds the arc at a
                // computed place, as k_dense_tie_export finds it: one gather to
                // confirm it instead of the search's dependent ones
                const int a0 = aux.rowPtr[ou], a1 = aux.rowPtr[ou + 1];
                if (a1 - a0 == aux.n - 1 && ou != ov) {
                    arc = a0 + (ov < ou ? ov : ov - 1);
                    found = aux.col[arc] == ov;
                }
            }
            if (found || (ou != ov && find_arc(aux, ou, ov, &arc))) {
                dev_add(acc + arc, s);
                ++issued;
            } else {                             // (never: a parent arc is an arc of the graph)
                dev_add(&out[7], 1ull);
            }
        }
        if (issued) atomicAdd(&issuedWg, issued);
        __syncthreads();                         // the slot is free for the next source
    }
    if (tid == 0) {
        if (claimedWg) dev_add(&out[5], claimedWg);
        if (issuedWg) dev_add(&out[6], issuedWg);
    }
}

void launch_tree_load_parents(const DevGraph& g, const DevGraph& gAux, const DevTable& tab,
                              const TreeParentsArgs& a, int grid, void* stream) {
    if (a.nSrc <= 0 || grid <= 0) return;
    const dim3 wgs((unsigned)(grid < a.nSrc ? grid : a.nSrc));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (a.vertexIds)
        hipLaunchKernelGGL(k_tree_load_parents<PAR_VERTEX>, wgs, dim3(TPAR_THREADS), 0, st, g, gAux, tab, a);
    else
        hipLaunchKernelGGL(k_tree_load_parents<PAR_INARC>, wgs, dim3(TPAR_THREADS), 0, st, g, gAux, tab, a);
}

void launch_paths_size(const DevGraph& gAux, const DevTable& tab, const PathsSizeArgs& a, void* stream) {
    if (a.count <= 0) return;
    hipLaunchKernelGGL(k_paths_size, dim3((unsigned)((a.count + 255) / 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), gAux, tab, a);
}

void launch_paths_scan(const int32_t* dLen, int32_t count, int64_t* dOff, void* stream) {
    hipLaunchKernelGGL(k_paths_scan, dim3(1), dim3(1024), 0, reinterpret_cast<hipStream_t>(stream), dLen,
                       count, dOff);
}

void launch_paths_flags(const DevTable& tab, const int32_t* dRows, int32_t nRows, uint8_t* dBuf,
                        bool restore, void* stream) {
    if (nRows <= 0) return;
    hipLaunchKernelGGL(k_paths_flags, dim3(nRows), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       tab, dRows, dBuf, restore ? 1 : 0);
}

void launch_paths_walk(const DevGraph& g, const PathsWalkArgs& a, void* stream) {
    if (a.nReqs <= 0) return;
    hipLaunchKernelGGL(k_paths_walk, dim3((unsigned)((a.nReqs + 255) / 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), g, a);
}

void launch_paths_hops(const DevGraph& gAux, const int64_t* dOff, int32_t count, int64_t entries,
                       const int32_t* dVerts, double* dHopLat, double* dHopRel, int32_t* dNFailed,
                       void* stream) {
    if (entries <= 0) return;
    hipLaunchKernelGGL(k_paths_hops, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), gAux, dOff, count, dVerts, dHopLat, dHopRel,
                       dNFailed);
}

void launch_paths_load(const DevGraph& gAux, const PathsLoadArgs& a, void* stream) {
    if (a.entries <= 0) return;
    const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    int slots = 8;                               // the largest power of two <= min(a.slots, LOAD_SLOTS_MAX)
    while (slots * 2 <= a.slots && slots * 2 <= LOAD_SLOTS_MAX) slots *= 2;
    const int64_t per = 256 * LOAD_PER_THREAD;
    hipLaunchKernelGGL(k_paths_load, dim3((unsigned)((a.entries + per - 1) / per)), dim3(256), 0, st, gAux, a.off,
                       a.count, a.verts, (const unsigned long long*)a.weight, a.nArcs, (unsigned long long*)a.acc,
                       a.nFailed, slots, (unsigned long long*)a.nIssued);
}

}  // namespace shdpe
