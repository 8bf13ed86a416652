// pe_attach.hip -- host attachment, batched on the device.
//
//   k_attach             _topology_findAttachmentVertex       topology.c:2248-2369
//                        _topology_findAttachmentVertexHelperHook      :2094-2217
//                        _topology_getLongestPrefixMatch               :2219-2246
//   shd_pe_attach_host   the same rule, one host, serial on the CPU
//   bwDown / bwUp        topology_attach                               :2398-2409
//
// The reference walks every vertex for every host (six igraph string lookups
// and four g_ascii_strcasecmp per visit).  With the strings interned
// (pe_graphml.cpp) a visit is four integer compares and the order-dependent
// parts have order-free forms (include/shd_pathengine.h states the rule):
//   - "clear the queues on the first exact IP match" (:2134-2159): the exact
//     matches are the candidates iff there is at least one;
//   - "first non-empty queue" (:2293-2317): an OR over the vertices of each
//     vertex's set-membership bits;
//   - the bestMatch loop (:2229-2243): first index of the maximum match, the
//     last candidate when the maximum is 0;
//   - popping chosenIndex + 1 heads (:2330-2333): the k-th candidate in vertex
//     order.
// One wave serves AT_G hosts (their hint words are wave-uniform, in SGPRs);
// its lanes take 64 consecutive vertices per step of the SoA vertex table
// (20 B per vertex: 2 MB at 10^5 vertices, L2-resident) and test each against
// every host of the group.  Up to three walks: (1) OR of the membership bits
// -> the set and the selection mode, (2) candidate count and the longest-
// prefix reduction, (3) ordered k-th selection with ballots.  Everything is
// wave-local: no atomics, no LDS, nothing decided by scheduling order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "shd_pathengine.h"

namespace shdpe {

struct AttachIn {        // one host, 32 B
    uint32_t ip;         // requestedIP: the hint if usable, else 0 (g_new0, :2255-2268)
    int32_t city, country, geo, type;   // -1 none, -2 matches nothing, else code
    uint32_t flags;      // AT_GIVEN | AT_REQ_USABLE
    double r;            // the would-be random_nextDouble
};
struct AttachOut {       // 16 B
    int32_t vertex, numCandidates;
    int32_t setMode;     // candidateSet | usedRandom << 8
    int32_t pad;
};
constexpr uint32_t AT_GIVEN = 1u, AT_REQ_USABLE = 2u;
constexpr uint32_t AT_EXACT = 0x100u;      // membership bit 8: exact IP match
constexpr int AT_G = 4;                    // hosts per wave

// :2127 / :2264 on the raw s_addr
__host__ __device__ inline bool usable_ip(uint32_t x) {
    return x != 0xffffffffu && x != 0u && x != 0x7f000001u;
}

// Bit s (0..7) = the vertex is in candidate set s (:2161-2214), bit 8 = it
// matches the requested IP exactly (:2134-2135).  code >= 0 && code == hint
// implies hint >= 0 (:2117-2120: attribute found, hint given, strings equal).
__host__ __device__ inline uint32_t member_bits(const AttachIn& h, uint32_t vip, int32_t c, int32_t k,
                                                int32_t g, int32_t t) {
    const uint32_t mC = c >= 0 && c == h.city, mK = k >= 0 && k == h.country;
    const uint32_t mG = g >= 0 && g == h.geo, mT = t >= 0 && t == h.type;
    const uint32_t ex = (h.flags & AT_REQ_USABLE) && usable_ip(vip) && vip == h.ip;
    return (mC & mT) | (mC << 1) | ((mK & mT) << 2) | (mK << 3) | ((mG & mT) << 4) | (mG << 5) |
           (mT << 6) | 0x80u | (ex << 8);
}
// walk 1 word: the membership bits, and for sets 0..7 "holds a usable vertex
// address" (numIPs* > 0) at bits 9..16
__host__ __device__ inline uint32_t walk1_bits(uint32_t m, uint32_t vip) {
    return m | (usable_ip(vip) ? (m & 0xffu) << 9 : 0u);
}
// the OR of walk1_bits over all vertices -> the set used (:2293-2317, 8 = the
// exact matches) and whether longest-prefix matching selects (:2324)
__host__ __device__ inline void decide(uint32_t orw, uint32_t flags, int* set, bool* prefix) {
    if (orw & AT_EXACT) { *set = 8; *prefix = false; return; }
    int s = 0;
    while (!((orw >> s) & 1u)) ++s;                   // bit 7 is always set
    const bool hasIp = (orw >> (9 + s)) & 1u;
    *set = s;
    *prefix = hasIp && (flags & (s < 7 ? AT_REQ_USABLE : AT_GIVEN));
}
// :2328-2329
__host__ __device__ inline int32_t chosen_index(int32_t numCandidates, double r) {
    return (int32_t)round((double)(numCandidates - 1) * r);
}

template <class T>
__device__ __forceinline__ T wave_uniform(T x) {
    return (T)__builtin_amdgcn_readfirstlane((int)x);
}

__global__ __launch_bounds__(256) void k_attach(const uint32_t* __restrict__ vIp,
                                                const int32_t* __restrict__ vCity,
                                                const int32_t* __restrict__ vCountry,
                                                const int32_t* __restrict__ vGeo,
                                                const int32_t* __restrict__ vType, int32_t n,
                                                const AttachIn* __restrict__ in, int32_t count,
                                                AttachOut* __restrict__ out) {
    const int wave = wave_uniform((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int32_t h0 = ((int32_t)blockIdx.x * 4 + wave) * AT_G;
    if (h0 >= count) return;                                   // uniform per wave
    AttachIn H[AT_G];
#pragma unroll
    for (int j = 0; j < AT_G; ++j) H[j] = in[min(h0 + j, count - 1)];   // tail: repeats, not written

    // ---- walk 1: which sets are non-empty / hold a usable address ---------
    uint32_t orw[AT_G];
#pragma unroll
    for (int j = 0; j < AT_G; ++j) orw[j] = 0u;
    for (int32_t base = 0; base < n; base += 64) {
        const int32_t v = min(base + lane, n - 1);             // tail lanes repeat the last vertex
        const uint32_t ip = vIp[v];
        const int32_t c = vCity[v], k = vCountry[v], g = vGeo[v], t = vType[v];
#pragma unroll
        for (int j = 0; j < AT_G; ++j) orw[j] |= walk1_bits(member_bits(H[j], ip, c, k, g, t), ip);
    }
    int set[AT_G];
    bool prefix[AT_G];
    bool allPlain = true;       // every host: all vertices, random choice
#pragma unroll
    for (int j = 0; j < AT_G; ++j) {
        uint32_t w = orw[j];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) w |= (uint32_t)__shfl_xor((int)w, o, 64);
        decide(wave_uniform(w), H[j].flags, &set[j], &prefix[j]);
        allPlain = allPlain && set[j] == 7 && !prefix[j];
    }

    // ---- walk 2: candidate count, longest-prefix reduction ----------------
    int32_t cnt[AT_G], winner[AT_G];
#pragma unroll
    for (int j = 0; j < AT_G; ++j) { cnt[j] = n; winner[j] = -1; }
    if (!allPlain) {
        uint32_t bm[AT_G];
        int32_t bi[AT_G], last[AT_G], c2[AT_G];
#pragma unroll
        for (int j = 0; j < AT_G; ++j) { bm[j] = 0u; bi[j] = -1; last[j] = -1; c2[j] = 0; }
        for (int32_t base = 0; base < n; base += 64) {
            const bool live = base + lane < n;
            const int32_t v = min(base + lane, n - 1);
            const uint32_t ip = vIp[v];
            const int32_t c = vCity[v], k = vCountry[v], g = vGeo[v], t = vType[v];
#pragma unroll
            for (int j = 0; j < AT_G; ++j) {
                const bool isIn = live && ((member_bits(H[j], ip, c, k, g, t) >> set[j]) & 1u);
                const uint32_t match = ~(ip ^ H[j].ip);                    // :2237
                c2[j] += isIn ? 1 : 0;
                // a lane sees its vertices in rising order: strict > keeps the first maximum
                if (isIn && (bi[j] < 0 || match > bm[j])) { bm[j] = match; bi[j] = v; }
                if (isIn) last[j] = v;
            }
        }
#pragma unroll
        for (int j = 0; j < AT_G; ++j) {
            // (match max, index min) as one u64 max; 0 = the lane has no candidate
            unsigned long long key =
                bi[j] < 0 ? 0ull : ((unsigned long long)bm[j] << 32) | (uint32_t)(0x7fffffff - bi[j]);
            int32_t cs = c2[j], lm = last[j];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned long long ok = __shfl_xor(key, o, 64);
                key = ok > key ? ok : key;
                cs += __shfl_xor(cs, o, 64);
                lm = max(lm, __shfl_xor(lm, o, 64));
            }
            cnt[j] = wave_uniform(cs);
            if (prefix[j]) {
                // a maximum of 0: every zero replaced the one before it (:2238), the last wins
                const int32_t first = 0x7fffffff - (int32_t)(uint32_t)(key & 0xffffffffull);
                winner[j] = wave_uniform((key >> 32) == 0ull ? lm : first);
            }
        }
    }

    // ---- walk 3: the k-th candidate in vertex order ------------------------
    int32_t kth[AT_G], run[AT_G];
    bool pending = false;
#pragma unroll
    for (int j = 0; j < AT_G; ++j) {
        kth[j] = 0;
        run[j] = 0;
        if (prefix[j]) continue;
        kth[j] = chosen_index(cnt[j], H[j].r);
        if (set[j] == 7) winner[j] = kth[j];                   // all vertices: the ordinal is the index
        else pending = true;
    }
    if (pending) {
        for (int32_t base = 0; base < n && pending; base += 64) {
            const bool live = base + lane < n;
            const int32_t v = min(base + lane, n - 1);
            const uint32_t ip = vIp[v];
            const int32_t c = vCity[v], k = vCountry[v], g = vGeo[v], t = vType[v];
            pending = false;
#pragma unroll
            for (int j = 0; j < AT_G; ++j) {
                if (winner[j] >= 0) continue;                  // uniform
                const bool isIn = live && ((member_bits(H[j], ip, c, k, g, t) >> set[j]) & 1u);
                const unsigned long long b = __ballot(isIn);
                const int32_t nb = __popcll(b);
                if (run[j] + nb > kth[j]) {
                    const int32_t rank = __popcll(b & ((1ull << lane) - 1ull));
                    const unsigned long long wb = __ballot(isIn && rank == kth[j] - run[j]);
                    winner[j] = base + (int32_t)__ffsll((long long)wb) - 1;
                } else {
                    run[j] += nb;
                    pending = true;
                }
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < AT_G; ++j)
            if (h0 + j < count) {
                AttachOut o;
                o.vertex = winner[j];
                o.numCandidates = cnt[j];
                o.setMode = set[j] | (prefix[j] ? 0 : 0x100);
                o.pad = 0;
                out[h0 + j] = o;
            }
    }
}

// ---- host side ------------------------------------------------------------
static int pack_host(const ShdPeAttachHints* h, int64_t i, AttachIn* o) {
    const double r = h->randomDouble[i];
    if (!(r >= 0.0 && r <= 1.0)) return SHD_PE_EINVAL;         // NaN fails both
    const bool given = h->ipHintGiven && h->ipHintGiven[i];
    const uint32_t ip = h->ipHint ? h->ipHint[i] : 0xffffffffu;
    const bool req = given && usable_ip(ip);
    o->ip = req ? ip : 0u;
    o->city = h->citycode ? h->citycode[i] : -1;
    o->country = h->countrycode ? h->countrycode[i] : -1;
    o->geo = h->geocode ? h->geocode[i] : -1;
    o->type = h->type ? h->type[i] : -1;
    o->flags = (given ? AT_GIVEN : 0u) | (req ? AT_REQ_USABLE : 0u);
    o->r = r;
    return SHD_PE_OK;
}

// (guint64) bandwidth (:2402, :2408); the reference asserts the value exists
static uint64_t bw_u64(const double* bw, int32_t v) {
    if (!bw || std::isnan(bw[v]) || bw[v] <= 0.0) return 0;
    return bw[v] >= 18446744073709551615.0 ? UINT64_MAX : (uint64_t)bw[v];
}

static void store_result(const ShdPeAttachResult* r, int64_t i, const AttachOut& o, const double* bwDown,
                         const double* bwUp) {
    r->vertex[i] = o.vertex;
    if (r->candidateSet) r->candidateSet[i] = (uint8_t)(o.setMode & 0xff);
    if (r->numCandidates) r->numCandidates[i] = o.numCandidates;
    if (r->usedRandom) r->usedRandom[i] = (uint8_t)((o.setMode >> 8) & 1);
    if (r->bwDown) r->bwDown[i] = bw_u64(bwDown, o.vertex);
    if (r->bwUp) r->bwUp[i] = bw_u64(bwUp, o.vertex);
}

}  // namespace shdpe

using namespace shdpe;

struct ShdPeAttach {
    int32_t device = 0, n = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    uint32_t* dIp = nullptr;
    int32_t* dCode[4] = {nullptr, nullptr, nullptr, nullptr};
    std::vector<double> bwDown, bwUp;           // empty = the graph has no such key
    int64_t chunk = 65536, cap = 0;
    AttachIn *hIn = nullptr, *dIn = nullptr;    // staging, `cap` hosts (hIn / hOut page-locked)
    AttachOut *hOut = nullptr, *dOut = nullptr;
    double msKernel = 0.0, msWall = 0.0;
};

static void attach_free_staging(ShdPeAttach* at) {
    if (at->hIn) (void)hipHostFree(at->hIn);
    if (at->hOut) (void)hipHostFree(at->hOut);
    if (at->dIn) (void)hipFree(at->dIn);
    if (at->dOut) (void)hipFree(at->dOut);
    at->hIn = at->dIn = nullptr;
    at->hOut = at->dOut = nullptr;
    at->cap = 0;
}

extern "C" void shd_pe_attach_free(ShdPeAttach* at) {
    if (!at) return;
    if (at->stream) {
        (void)hipSetDevice(at->device);
        attach_free_staging(at);
        if (at->dIp) (void)hipFree(at->dIp);
        for (int32_t* p : at->dCode)
            if (p) (void)hipFree(p);
        if (at->ev0) (void)hipEventDestroy(at->ev0);
        if (at->ev1) (void)hipEventDestroy(at->ev1);
        (void)hipStreamDestroy(at->stream);
    }
    delete at;
}

extern "C" int shd_pe_attach_new(const ShdPeVertexAttrs* va, int32_t device, ShdPeAttach** out) {
    if (!out) return SHD_PE_EINVAL;
    *out = nullptr;
    if (!va || va->nVertices <= 0) return SHD_PE_EINVAL;
    int nDev = 0;
    if (hipGetDeviceCount(&nDev) != hipSuccess || device < 0 || device >= nDev) return SHD_PE_ENODEV;
    if (hipSetDevice(device) != hipSuccess) return SHD_PE_ENODEV;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return SHD_PE_ENODEV;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return SHD_PE_ENODEV;
    ShdPeAttach* at = new (std::nothrow) ShdPeAttach();
    if (!at) return SHD_PE_ENOMEM;
    at->device = device;
    at->n = va->nVertices;
    if (hipStreamCreateWithFlags(&at->stream, hipStreamNonBlocking) != hipSuccess) {
        at->stream = nullptr;
        delete at;
        return SHD_PE_ENODEV;
    }
    int rc = SHD_PE_OK;
    try {
        const size_t n = (size_t)at->n;
        if (va->bandwidthDown) at->bwDown.assign(va->bandwidthDown, va->bandwidthDown + n);
        if (va->bandwidthUp) at->bwUp.assign(va->bandwidthUp, va->bandwidthUp + n);
        // a key the graph lacks: no vertex has the attribute
        std::vector<uint32_t> none(n, 0xffffffffu);
        const void* src[5] = {va->ip, va->citycode, va->countrycode, va->geocode, va->type};
        void* dst[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
        if (hipEventCreate(&at->ev0) != hipSuccess || hipEventCreate(&at->ev1) != hipSuccess) rc = SHD_PE_EHIP;
        for (int a = 0; a < 5 && !rc; ++a) {
            if (hipMalloc(&dst[a], n * 4) != hipSuccess) { dst[a] = nullptr; rc = SHD_PE_ENOMEM; break; }
            if (a == 0) at->dIp = (uint32_t*)dst[a];
            else at->dCode[a - 1] = (int32_t*)dst[a];
            if (hipMemcpy(dst[a], src[a] ? src[a] : none.data(), n * 4, hipMemcpyHostToDevice) != hipSuccess)
                rc = SHD_PE_EHIP;
        }
    } catch (const std::bad_alloc&) {
        rc = SHD_PE_ENOMEM;
    }
    if (rc) { shd_pe_attach_free(at); return rc; }
    *out = at;
    return SHD_PE_OK;
}

extern "C" int shd_pe_attach_set_chunk(ShdPeAttach* at, int64_t hostsPerChunk) {
    if (!at || hostsPerChunk <= 0 || hostsPerChunk > ((int64_t)1 << 24)) return SHD_PE_EINVAL;
    at->chunk = hostsPerChunk;
    return SHD_PE_OK;
}

extern "C" int shd_pe_attach_timing(const ShdPeAttach* at, double* ms) {
    if (!at || !ms) return SHD_PE_EINVAL;
    ms[0] = at->msKernel;
    ms[1] = at->msWall;
    return SHD_PE_OK;
}

#define ATCHK(x)                                   \
    do {                                           \
        if ((x) != hipSuccess) return SHD_PE_EHIP; \
    } while (0)

extern "C" int shd_pe_attach_hosts(ShdPeAttach* at, const ShdPeAttachHints* h, const ShdPeAttachResult* r) {
    if (!at || !h || !r || h->count < 0) return SHD_PE_EINVAL;
    if (h->count == 0) return SHD_PE_OK;
    if (!r->vertex || !h->randomDouble) return SHD_PE_EINVAL;
    for (int64_t i = 0; i < h->count; ++i)
        if (!(h->randomDouble[i] >= 0.0 && h->randomDouble[i] <= 1.0)) return SHD_PE_EINVAL;
    const auto t0 = std::chrono::steady_clock::now();
    ATCHK(hipSetDevice(at->device));
    const int64_t ch = std::min<int64_t>(h->count, at->chunk);
    if (at->cap < ch) {
        attach_free_staging(at);
        if (hipHostMalloc((void**)&at->hIn, (size_t)ch * sizeof(AttachIn)) != hipSuccess ||
            hipHostMalloc((void**)&at->hOut, (size_t)ch * sizeof(AttachOut)) != hipSuccess ||
            hipMalloc((void**)&at->dIn, (size_t)ch * sizeof(AttachIn)) != hipSuccess ||
            hipMalloc((void**)&at->dOut, (size_t)ch * sizeof(AttachOut)) != hipSuccess) {
            attach_free_staging(at);
            return SHD_PE_ENOMEM;
        }
        at->cap = ch;
    }
    const double* bwD = at->bwDown.empty() ? nullptr : at->bwDown.data();
    const double* bwU = at->bwUp.empty() ? nullptr : at->bwUp.data();
    double msK = 0.0;
    for (int64_t c0 = 0; c0 < h->count; c0 += ch) {
        const int32_t c = (int32_t)std::min<int64_t>(ch, h->count - c0);
        for (int32_t i = 0; i < c; ++i) {
            const int rc = pack_host(h, c0 + i, &at->hIn[i]);
            if (rc) return rc;
        }
        ATCHK(hipMemcpyAsync(at->dIn, at->hIn, (size_t)c * sizeof(AttachIn), hipMemcpyHostToDevice, at->stream));
        const int32_t waves = (c + AT_G - 1) / AT_G;
        ATCHK(hipEventRecord(at->ev0, at->stream));
        hipLaunchKernelGGL(k_attach, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, at->stream, at->dIp,
                           at->dCode[0], at->dCode[1], at->dCode[2], at->dCode[3], at->n, at->dIn, c, at->dOut);
        ATCHK(hipGetLastError());
        ATCHK(hipEventRecord(at->ev1, at->stream));
        ATCHK(hipMemcpyAsync(at->hOut, at->dOut, (size_t)c * sizeof(AttachOut), hipMemcpyDeviceToHost, at->stream));
        ATCHK(hipStreamSynchronize(at->stream));
        float ms = 0.f;
        ATCHK(hipEventElapsedTime(&ms, at->ev0, at->ev1));
        msK += ms;
        for (int32_t i = 0; i < c; ++i) {
            const AttachOut& o = at->hOut[i];
            if (o.vertex < 0 || o.vertex >= at->n) return SHD_PE_EHIP;      // never: a set is never empty
            store_result(r, c0 + i, o, bwD, bwU);
        }
    }
    at->msKernel = msK;
    at->msWall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return SHD_PE_OK;
}

// One host on the CPU: two passes over the vertices in vertex order with the
// helpers the kernel uses, so the batched and the one-query form cannot drift
// apart.
extern "C" int shd_pe_attach_host(const ShdPeVertexAttrs* va, const ShdPeAttachHints* h, int64_t i,
                                  const ShdPeAttachResult* r) {
    if (!va || !h || !r || !r->vertex || !h->randomDouble || va->nVertices <= 0 || i < 0 || i >= h->count)
        return SHD_PE_EINVAL;
    AttachIn H;
    const int rc = pack_host(h, i, &H);
    if (rc) return rc;
    const int32_t n = va->nVertices;
    auto ip = [&](int32_t v) { return va->ip ? va->ip[v] : 0xffffffffu; };
    auto bits = [&](int32_t v) {
        return member_bits(H, ip(v), va->citycode ? va->citycode[v] : -1,
                           va->countrycode ? va->countrycode[v] : -1, va->geocode ? va->geocode[v] : -1,
                           va->type ? va->type[v] : -1);
    };
    uint32_t orw = 0;
    for (int32_t v = 0; v < n; ++v) orw |= walk1_bits(bits(v), ip(v));
    int set;
    bool prefix;
    decide(orw, H.flags, &set, &prefix);
    int32_t cnt = 0, first = -1, last = -1;
    uint32_t bm = 0;
    for (int32_t v = 0; v < n; ++v) {
        if (!((bits(v) >> set) & 1u)) continue;
        ++cnt;
        const uint32_t match = ~(ip(v) ^ H.ip);
        if (first < 0 || match > bm) { bm = match; first = v; }
        last = v;
    }
    AttachOut o;
    o.numCandidates = cnt;
    o.setMode = set | (prefix ? 0 : 0x100);
    o.pad = 0;
    if (prefix) {
        o.vertex = bm == 0 ? last : first;
    } else {
        int32_t k = chosen_index(cnt, H.r);
        o.vertex = -1;
        for (int32_t v = 0; v < n; ++v)
            if (((bits(v) >> set) & 1u) && k-- == 0) { o.vertex = v; break; }
    }
    store_result(r, i, o, va->bandwidthDown, va->bandwidthUp);
    return SHD_PE_OK;
}
