// pe_rows.hip -- row transport of the MI355X Shadow path engine: everything
// that moves finished table rows.  Out of the device: shd_pe_get_row(s),
// shd_pe_copy_rows_device, shd_pe_row_checksums, shd_pe_fill_rowstore(_ex),
// shd_pe_fill_rowstore_shards;
// between devices: shd_pe_gather, shd_pe_put_rows, shd_pe_comm_*.
//
// A table is the parallel field arrays of TABLE_FIELDS (pe_device.hpp), and a
// transfer moves the same row range of every field both sides have: each copy
// below is one for_each_field over two DevTable views -- a device table, a
// caller's host or device buffers, a staging block -- with the copy it wants.
#include <sys/mman.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "pe_engine.hpp"
#include "pe_fill.hpp"

using namespace shdpe;

// A contiguous run of table rows readable from one device table.
struct Piece {
    const DevTable* tab;
    hipStream_t stream;
    int device;
    int32_t start, count;   // table positions
};

static int table_pieces(ShdPe* pe, int32_t start, int32_t count, std::vector<Piece>& out) {
    out.clear();
    if (pe->gathered) {
        Shard* s = pe->shards[0].get();
        out.push_back(Piece{&s->full, s->copyStream, s->device, start, count});
        return SHD_PE_OK;
    }
    int32_t p = start;
    while (p < start + count) {
        Shard* s = owner_of(pe, p);
        if (!s || !s->tableReady) return SHD_PE_ENOTOWNED;
        const int32_t end = std::min(start + count, s->rowStart + s->rowCount);
        out.push_back(Piece{&s->tab, s->copyStream, s->device, p, end - p});
        p = end;
    }
    return SHD_PE_OK;
}

static int get_rows_staged(ShdPe* pe, int32_t start, int32_t count, double* lat, double* rel,
                           int32_t* hops, int32_t* pred, uint8_t* flags);

extern "C" int shd_pe_get_row(ShdPe* pe, int32_t srcVertex, double* lat, double* rel,
                              int32_t* hops, int32_t* pred, uint8_t* flags) {
    if (!pe || srcVertex < 0 || srcVertex >= pe->hg.n) return SHD_PE_EINVAL;
    const int32_t p = pe->posOf[srcVertex];
    if (p < 0) return SHD_PE_ENOTATTACHED;
    if (pred && !pe->opt.storePred) return SHD_PE_EINVAL;
    int rc = ensure_rows(pe, p, 1);
    if (rc) return rc;
    return get_rows_staged(pe, p, 1, lat, rel, hops, pred, flags);
}

// Host memcpy split over up to 8 threads: the drain of a staging block into
// caller (pageable, often freshly allocated) memory runs at one core's
// page-fault + copy rate otherwise.
static void par_memcpy(void* dst, const void* src, size_t bytes) {
    const size_t minChunk = (size_t)2 << 20;
    const unsigned hc = std::thread::hardware_concurrency();
    const int nt = (int)std::max<size_t>(1, std::min<size_t>({(size_t)8, hc ? hc : 1, bytes / minChunk}));
    if (nt <= 1) { std::memcpy(dst, src, bytes); return; }
    std::vector<std::thread> th;
    const size_t per = (bytes + nt - 1) / nt;
    for (int t = 1; t < nt; ++t) {
        const size_t o = per * t;
        if (o >= bytes) break;
        th.emplace_back([=]() { std::memcpy((char*)dst + o, (const char*)src + o, std::min(per, bytes - o)); });
    }
    std::memcpy(dst, src, std::min(per, bytes));
    for (auto& x : th) x.join();
}

// Page-locked host memory the device can DMA into (hipHostMalloc or
// hipHostRegister): such caller buffers skip the staging copy.
static bool is_pinned(const void* p) {
    if (!p) return true;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return at.type == hipMemoryTypeHost && at.hostPointer != nullptr;
}

// A caller's buffers (host or device; any may be null) as a view: they hold
// rows from table position `start`.
static DevTable caller_view(const double* lat, const double* rel, const int32_t* hops, const int32_t* pred,
                            const uint8_t* flags, size_t T, int32_t start) {
    return DevTable{const_cast<double*>(lat), const_cast<double*>(rel), const_cast<int32_t*>(hops),
                    const_cast<int32_t*>(pred), const_cast<uint8_t*>(flags), (int64_t)T, start};
}

// for_each_field's copy as a hipMemcpyAsync of `kind` on `stream`.
static auto async_copy(hipMemcpyKind kind, hipStream_t stream) {
    return [=](void* dst, const void* src, int64_t bytes, int) -> int {
        HIPCHK(hipMemcpyAsync(dst, src, (size_t)bytes, kind, stream));
        return SHD_PE_OK;
    };
}

// Rows [start, start+count) -> caller host buffers.  Pinned caller buffers
// take the DMA straight (one copy per field and table piece); otherwise two
// pinned staging buffers: block b's field copies run on the copy stream
// while host threads copy block b-1 out of the other buffer.
// The walk skips a field either side lacks, so a `pred` buffer against a
// table without storePred would come back unwritten: every entry point
// refuses that with SHD_PE_EINVAL before it gets here, and a new one must too.
static int get_rows_staged(ShdPe* pe, int32_t start, int32_t count, double* lat, double* rel,
                           int32_t* hops, int32_t* pred, uint8_t* flags) {
    const size_t T = pe->attached.size();
    const size_t perRow = T * (size_t)table_cell_bytes();
    const DevTable out = caller_view(lat, rel, hops, pred, flags, T, start);
    std::lock_guard<std::mutex> lk(pe->copyMu);
    std::vector<Piece> pieces;
    int rc = table_pieces(pe, start, count, pieces);
    if (rc) return rc;
    if (is_pinned(lat) && is_pinned(rel) && is_pinned(hops) && is_pinned(pred) && is_pinned(flags)) {
        for (const Piece& pc : pieces) {
            HIPCHK(hipSetDevice(pc.device));
            if ((rc = for_each_field(*pc.tab, out, pc.start, pc.count,
                                     async_copy(hipMemcpyDeviceToHost, pc.stream))))
                return rc;
        }
        for (const Piece& pc : pieces) {
            HIPCHK(hipSetDevice(pc.device));
            HIPCHK(hipStreamSynchronize(pc.stream));
        }
        return SHD_PE_OK;
    }
    if (!pe->stage[0]) {
        const size_t want = std::max<size_t>(perRow, (size_t)64 << 20);
        for (auto& h : pe->stage)
            HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&h), want, hipHostMallocPortable));
        pe->stageBytes = want;
    }
    // (rows per block from the full row size, whatever fields are asked for)
    const int32_t B = (int32_t)std::max<size_t>(1, pe->stageBytes / perRow);
    for (const Piece& pc : pieces) {
        HIPCHK(hipSetDevice(pc.device));
        struct Blk { int32_t r0, n; };   // r0: table position
        // a block in its staging buffer: the wanted fields packed back to back
        auto staged = [&](int buf, Blk b) { return stage_view(pe->stage[buf], b.r0, b.n, out); };
        auto issue = [&](int buf, Blk b) {
            return for_each_field(*pc.tab, staged(buf, b), b.r0, b.n, async_copy(hipMemcpyDeviceToHost, pc.stream));
        };
        auto drain = [&](int buf, Blk b) {
            (void)for_each_field(staged(buf, b), out, b.r0, b.n, [](void* dst, const void* src, int64_t bytes, int) {
                par_memcpy(dst, src, (size_t)bytes);
                return 0;
            });
        };
        hipEvent_t done[2];
        HIPCHK(hipEventCreateWithFlags(&done[0], hipEventDisableTiming));
        if (hipEventCreateWithFlags(&done[1], hipEventDisableTiming) != hipSuccess) {
            (void)hipEventDestroy(done[0]);
            return SHD_PE_EHIP;
        }
        Blk prev{0, 0};
        int buf = 0;
        for (int32_t r0 = 0; r0 < pc.count && rc == SHD_PE_OK; r0 += B) {
            const Blk cur{pc.start + r0, std::min(B, pc.count - r0)};
            if ((rc = issue(buf, cur)) == SHD_PE_OK &&
                hipEventRecord(done[buf], pc.stream) != hipSuccess)
                rc = SHD_PE_EHIP;
            if (rc == SHD_PE_OK && prev.n) {
                if (hipEventSynchronize(done[buf ^ 1]) != hipSuccess) rc = SHD_PE_EHIP;
                else drain(buf ^ 1, prev);
            }
            prev = cur;
            buf ^= 1;
        }
        if (rc == SHD_PE_OK && prev.n) {
            if (hipEventSynchronize(done[buf ^ 1]) != hipSuccess) rc = SHD_PE_EHIP;
            else drain(buf ^ 1, prev);
        }
        (void)hipStreamSynchronize(pc.stream);
        (void)hipEventDestroy(done[0]);
        (void)hipEventDestroy(done[1]);
        if (rc) return rc;
    }
    return rc;
}

extern "C" int shd_pe_get_rows(ShdPe* pe, int32_t start, int32_t count, double* lat, double* rel,
                               int32_t* hops, int32_t* pred, uint8_t* flags) {
    if (!pe || start < 0 || count < 0 || (int64_t)start + count > (int64_t)pe->attached.size())
        return SHD_PE_EINVAL;
    if (pred && !pe->opt.storePred) return SHD_PE_EINVAL;
    if (count == 0) return SHD_PE_OK;
    int rc = ensure_rows(pe, start, count);
    if (rc) return rc;
    return get_rows_staged(pe, start, count, lat, rel, hops, pred, flags);
}

extern "C" int shd_pe_host_alloc(int64_t bytes, void** out) {
    if (!out || bytes <= 0) return SHD_PE_EINVAL;
    *out = nullptr;
    if (hipHostMalloc(out, (size_t)bytes, hipHostMallocPortable) != hipSuccess) {
        *out = nullptr;
        return SHD_PE_ENOMEM;
    }
    return SHD_PE_OK;
}

extern "C" void shd_pe_host_free(void* p) {
    if (p) (void)hipHostFree(p);
}

extern "C" int shd_pe_copy_rows_device(ShdPe* pe, int32_t start, int32_t count, double* dLat,
                                       double* dRel, int32_t* dHops, uint8_t* dFlags) {
    if (!pe || start < 0 || count < 0 || (int64_t)start + count > (int64_t)pe->attached.size())
        return SHD_PE_EINVAL;
    if (count == 0) return SHD_PE_OK;
    int rc = ensure_rows(pe, start, count);       // same contract as shd_pe_get_rows
    if (rc) return rc;
    // table_pieces reads gathered / the full table, which shd_pe_gather
    // writes under copyMu
    std::lock_guard<std::mutex> lk(pe->copyMu);
    std::vector<Piece> pieces;
    if ((rc = table_pieces(pe, start, count, pieces))) return rc;
    const DevTable out = caller_view(dLat, dRel, dHops, nullptr, dFlags, pe->attached.size(), start);
    for (const Piece& pc : pieces) {
        HIPCHK(hipSetDevice(pc.device));
        if ((rc = for_each_field(*pc.tab, out, pc.start, pc.count, async_copy(hipMemcpyDeviceToDevice, pc.stream))))
            return rc;
        HIPCHK(hipStreamSynchronize(pc.stream));
    }
    return SHD_PE_OK;
}

extern "C" int shd_pe_row_checksums(ShdPe* pe, int32_t start, int32_t count, uint64_t* out) {
    if (!pe || !out || start < 0 || count < 0 || (int64_t)start + count > (int64_t)pe->attached.size())
        return SHD_PE_EINVAL;
    if (count == 0) return SHD_PE_OK;
    int rc = ensure_rows(pe, start, count);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(pe->copyMu);
    std::vector<Piece> pieces;
    if ((rc = table_pieces(pe, start, count, pieces))) return rc;
    for (const Piece& pc : pieces) {
        HIPCHK(hipSetDevice(pc.device));
        uint64_t* d = nullptr;
        if (hipMalloc(&d, (size_t)pc.count * 8) != hipSuccess) return SHD_PE_ENOMEM;
        launch_row_checksums(*pc.tab, (int64_t)pc.start - pc.tab->rowStart, pc.count, d, pc.stream);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess)
            e = hipMemcpyAsync(out + (pc.start - start), d, (size_t)pc.count * 8, hipMemcpyDeviceToHost,
                               pc.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(pc.stream);
        (void)hipFree(d);
        if (e != hipSuccess) return SHD_PE_EHIP;
    }
    return SHD_PE_OK;
}

// The whole-table path-cache fill (topology.c:1805-1864 for every row, in
// position order) as one device pass: k_pack_rowstore builds the row
// store's own image of its triangular rows (2.3 GB at C4 vs 7.8 GB of
// rows), one DMA lands it in page-locked host memory the store adopts.
//
// The host image (2.3 GB at C4) is anonymous memory with transparent huge
// pages, first-touched by 16 threads and then registered with the device
// (page-locked): hipHostMalloc of the same size took 430 ms, most of it
// faulting and zeroing 4-KB pages on one thread.  When the rows still have
// to be computed, that preparation runs on a host thread while the device
// computes them.
struct HostImage {
    void* p = nullptr;
    size_t bytes = 0;
    bool registered = false;
    double msTouch = 0.0, msRegister = 0.0;
    ~HostImage();
};

// (regFlags: hipHostRegisterPortable when several devices DMA into the image)
static void host_image_prepare(HostImage* im, size_t bytes, unsigned regFlags) {
    const auto t0 = std::chrono::steady_clock::now();
    void* p = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (p == MAP_FAILED) return;
    (void)madvise(p, bytes, MADV_HUGEPAGE);
    const size_t nt = 16, chunk = ((bytes + nt - 1) / nt + 4095) & ~(size_t)4095;
    std::vector<std::thread> th;
    for (size_t t = 0; t < nt; ++t)
        th.emplace_back([=] {
            unsigned char* q = static_cast<unsigned char*>(p);
            for (size_t o = t * chunk; o < std::min(bytes, (t + 1) * chunk); o += 4096) q[o] = 0;
        });
    for (auto& x : th) x.join();
    im->p = p;
    im->bytes = bytes;
    const auto t1 = std::chrono::steady_clock::now();
    im->registered = hipHostRegister(p, bytes, regFlags) == hipSuccess;
    const auto t2 = std::chrono::steady_clock::now();
    im->msTouch = std::chrono::duration<double, std::milli>(t1 - t0).count();
    im->msRegister = std::chrono::duration<double, std::milli>(t2 - t1).count();
}

static void host_image_release(HostImage* im) {
    if (!im->p) return;
    if (im->registered) (void)hipHostUnregister(im->p);
    (void)munmap(im->p, im->bytes);
    im->p = nullptr;
}

HostImage::~HostImage() { host_image_release(this); }   // every exit path of fill_rowstore

static void host_image_free_cb(void* ctx, void* p) {
    (void)p;
    delete static_cast<HostImage*>(ctx);
}

// posOf[] on the shard's device (the current one), once per shard; caller holds copyMu
static int ensure_pos_of(ShdPe* pe, Shard* s) {
    if (s->dPosOf) return SHD_PE_OK;
    void* d = nullptr;
    if (hipMalloc(&d, pe->posOf.size() * 4) != hipSuccess) return SHD_PE_ENOMEM;
    if (hipMemcpy(d, pe->posOf.data(), pe->posOf.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(d);
        return SHD_PE_EHIP;
    }
    s->dPosOf = static_cast<int32_t*>(d);
    return SHD_PE_OK;
}

// The pack kernel's variant for a fill: 0 the non-direct rule alone (no flag,
// or DIRECT_PAIRS without a pair topology.c:2019-2021 serves directly), 1 a
// complete graph's direct table (k_direct_rows wrote the entries), 2 the
// adjacency rule (prefersDirectPaths; a complete graph whose table holds
// Dijkstra rows, forceMode)
static int fill_pack_mode(const ShdPe* pe, int32_t fillFlags) {
    if (pe->hg.isComplete) return pe->mode == 2 ? 1 : 2;
    return (fillFlags & SHD_PE_FILL_PREFER_DIRECT) ? 2 : 0;
}

extern "C" int shd_pe_fill_rowstore_ex(ShdPe* pe, ShdRowStore* st, int32_t fillFlags,
                                       int32_t* rowResult, double* msOut) {
    if (!pe || !st) return SHD_PE_EINVAL;
    if (fillFlags & ~(SHD_PE_FILL_PREFER_DIRECT | SHD_PE_FILL_DIRECT_PAIRS)) return SHD_PE_EINVAL;
    if (shd_rowstore_size(st) != 0) return SHD_PE_EINVAL;   // (adopt_image re-checks under its lock)
    const int32_t T = (int32_t)pe->attached.size();
    const bool wantDirect = (fillFlags & SHD_PE_FILL_DIRECT_PAIRS) != 0;
    const int packMode = fill_pack_mode(pe, fillFlags);
    if (packMode == 2 && pack_adj_lds_bytes(T, pe->hg.directed) < 0) return SHD_PE_ETOOBIG;
    static const char* const modeName[3] = {"plain", "complete-direct", "prefer-direct"};
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    std::vector<int64_t> off((size_t)T + 1);
    shd_rowstore_image_layout(T, off.data());
    const size_t bytes = (size_t)off[(size_t)T];
    // a complete graph stores no non-direct path (:1321): only its direct pairs
    const bool pack = !pe->hg.isComplete || wantDirect;
    const auto t0 = now();
    std::unique_ptr<HostImage> him(new HostImage);
    std::thread prep;
    if (pack) prep = std::thread(host_image_prepare, him.get(), bytes, (unsigned)hipHostRegisterDefault);   // beside the compute
    int rc = ensure_rows(pe, 0, T);
    const auto tc = now();
    if (prep.joinable()) prep.join();
    if (std::getenv("SHDPE_FILL_LOG"))
        std::fprintf(stderr, "[shdpe] fill_rowstore (%s%s): compute %.1f ms, image %.2f GB touch %.1f ms + "
                     "register %.1f ms (%s), join wait %.1f ms\n", pack ? modeName[packMode] : "nothing stored",
                     pack && wantDirect ? ", direct pairs" : "", ms(t0, tc), bytes / 1e9, him->msTouch,
                     him->msRegister, him->registered ? "registered" : "NOT registered", ms(tc, now()));
    if (rc) return rc;
    if (pack && !him->p) return SHD_PE_ENOMEM;
    std::lock_guard<std::mutex> lk(pe->copyMu);
    const DevTable* tab = nullptr;
    Shard* s = pe->shards[0].get();
    if (pe->gathered) tab = &s->full;
    else if (pe->G == 1) tab = &s->tab;
    else return SHD_PE_ENOTOWNED;          // rows spread over shards: gather first
    if (hipSetDevice(s->device) != hipSuccess) return SHD_PE_EHIP;
    if (pack && packMode == 2 && (rc = ensure_pos_of(pe, s))) return rc;
    void *dImg = nullptr, *dOff = nullptr, *dAcc = nullptr, *dAll = nullptr;
    void* const hImg = him->p;
    struct Free {   // device temporaries, every exit path (the host image: ~HostImage)
        void** p[4];
        ~Free() {
            for (void** q : p) if (*q) (void)hipFree(*q);
        }
    } fr{{&dImg, &dOff, &dAcc, &dAll}};
    if ((pack && hipMalloc(&dImg, bytes) != hipSuccess) ||
        hipMalloc(&dOff, off.size() * 8) != hipSuccess || hipMalloc(&dAcc, 16) != hipSuccess ||
        hipMalloc(&dAll, (size_t)T * 4) != hipSuccess)
        return SHD_PE_ENOMEM;
    const auto t1 = now();
    const unsigned long long acc0[2] = {0ull, 0x7FF0000000000000ull};
    unsigned long long acc[2] = {0ull, 0ull};
    hipError_t e = hipMemcpyAsync(dOff, off.data(), off.size() * 8, hipMemcpyHostToDevice, s->copyStream);
    if (e == hipSuccess) e = hipMemcpyAsync(dAcc, acc0, 16, hipMemcpyHostToDevice, s->copyStream);
    if (e == hipSuccess) {
        // the whole table: the one view with no rows behind it, so no needs
        if (pack && launch_pack_rowstore(*tab, PackView{0, T}, (const int64_t*)dOff, (uint8_t*)dImg,
                                         (unsigned long long*)dAcc, nullptr, packMode, &s->dgAux, s->dPosOf,
                                         wantDirect, pe->hg.isComplete, s->copyStream))
            return SHD_PE_ETOOBIG;
        launch_rows_all_success(*tab, T, (int32_t*)dAll, s->copyStream);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s->copyStream);
    const auto t2 = now();
    if (e == hipSuccess && pack) e = hipMemcpyAsync(hImg, dImg, bytes, hipMemcpyDeviceToHost, s->copyStream);
    if (e == hipSuccess) e = hipMemcpyAsync(acc, dAcc, 16, hipMemcpyDeviceToHost, s->copyStream);
    if (e == hipSuccess && rowResult)
        e = hipMemcpyAsync(rowResult, dAll, (size_t)T * 4, hipMemcpyDeviceToHost, s->copyStream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->copyStream);
    const auto t3 = now();
    if (e != hipSuccess) return SHD_PE_EHIP;
    if (pack) {
        double mn;
        std::memcpy(&mn, &acc[1], 8);
        rc = shd_rowstore_adopt_image(st, hImg, (int64_t)bytes, host_image_free_cb, him.get(),
                                      (int64_t)acc[0], mn);
        if (rc) return rc;
        him.release();   // the store owns it now
    }
    if (msOut) { msOut[0] = ms(t0, t1); msOut[1] = ms(t1, t2); msOut[2] = ms(t2, t3); }
    return SHD_PE_OK;
}

extern "C" int shd_pe_fill_rowstore(ShdPe* pe, ShdRowStore* st, int32_t* rowResult, double* msOut) {
    return shd_pe_fill_rowstore_ex(pe, st, 0, rowResult, msOut);
}

// ---------------------------------------------------------------------------
// The same fill without a gather ("a per-GPU D2H of its own
// shard replaces the gather"): every row shard of an in-process engine packs
// its own triangular rows [lo, hi) from its own table on its own device and
// DMAs the segment to its place off[lo] in the one host image.  A slot of row
// a is decided by row a alone unless its forward entry is not used; then the
// rule looks at entry (b, a), and for b >= hi that row is another shard's: a
// need (k_pack_rowstore).  Needs go to the owner of row b and come back as
// (ok, lat, rel) through pinned host staging -- no peer access, no full table
// -- in rounds of at most needBudgetBytes, and pe_fill.cpp writes the answers
// into the landed image before the store adopts it.
// ---------------------------------------------------------------------------
namespace {

// One shard's device temporaries of a call, with their running sum; freed on
// every exit path.
struct DevTemps {
    int device = 0;
    std::vector<std::pair<void*, int64_t>> blocks;
    int64_t cur = 0, peak = 0;
    void* take(int64_t bytes) {
        void* q = nullptr;
        if (hipSetDevice(device) != hipSuccess || hipMalloc(&q, (size_t)std::max<int64_t>(bytes, 16)) != hipSuccess)
            return nullptr;
        blocks.push_back({q, bytes});
        cur += bytes;
        peak = std::max(peak, cur);
        return q;
    }
    void release(size_t keep) {
        while (blocks.size() > keep) {
            (void)hipSetDevice(device);
            (void)hipFree(blocks.back().first);
            cur -= blocks.back().second;
            blocks.pop_back();
        }
    }
    ~DevTemps() { release(0); }
};

struct PinnedBlock {
    void* p = nullptr;
    ~PinnedBlock() { if (p) (void)hipHostFree(p); }
};

// What a shard keeps on its device from the pack to the end of its rounds.
struct ShardFill {
    Shard* s = nullptr;
    PackView pv{0, 0};
    int64_t segBytes = 0;
    uint8_t* dImg = nullptr;
    int64_t* dOff = nullptr;
    unsigned long long* dAcc = nullptr;
    int32_t *dAll = nullptr, *dNeed = nullptr;
    unsigned long long acc[2] = {0ull, 0ull};
    std::vector<int32_t> needCount, rounds;
};

}  // namespace

extern "C" int shd_pe_fill_rowstore_shards(ShdPe* pe, ShdRowStore* st, int32_t fillFlags,
                                           int64_t needBudgetBytes, int32_t* rowResult,
                                           ShdPeFillShardsInfo* info) {
    if (!pe || !st) return SHD_PE_EINVAL;
    if (fillFlags & ~(SHD_PE_FILL_PREFER_DIRECT | SHD_PE_FILL_DIRECT_PAIRS)) return SHD_PE_EINVAL;
    if (shd_rowstore_size(st) != 0) return SHD_PE_EINVAL;
    const int32_t T = (int32_t)pe->attached.size();
    const bool wantDirect = (fillFlags & SHD_PE_FILL_DIRECT_PAIRS) != 0;
    const int packMode = fill_pack_mode(pe, fillFlags);
    if (packMode == 2 && pack_adj_lds_bytes(T, pe->hg.directed) < 0) return SHD_PE_ETOOBIG;
    const bool pack = !pe->hg.isComplete || wantDirect;
    std::vector<int64_t> off((size_t)T + 1);
    shd_rowstore_image_layout(T, off.data());
    const size_t bytes = (size_t)off[(size_t)T];
    ShdPeFillShardsInfo inf{};
    bool full;
    {
        std::lock_guard<std::mutex> lk(pe->copyMu);
        full = pe->G == 1 || pe->gathered;
    }
    if (full) {   // one table serves the call: the _ex path
        double ms[3] = {0.0, 0.0, 0.0};
        const int rc = shd_pe_fill_rowstore_ex(pe, st, fillFlags, rowResult, ms);
        if (rc) return rc;
        inf.shards = 1;
        inf.fromFullTable = 1;
        inf.deviceBytesPeak = (int64_t)(pack ? bytes : 0) + (int64_t)off.size() * 8 + 16 + (int64_t)T * 4;
        inf.msCompute = ms[0];
        inf.msPack = ms[1];
        inf.msDma = ms[2];
        if (info) *info = inf;
        return SHD_PE_OK;
    }
    // rows of other processes' engines: their store is theirs
    if (pe->opt.shardCount > 1 || (int)pe->shards.size() != pe->G) return SHD_PE_ENOTOWNED;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    const auto t0 = now();
    std::unique_ptr<HostImage> him(new HostImage);
    std::thread prep;
    if (pack) prep = std::thread(host_image_prepare, him.get(), bytes, (unsigned)hipHostRegisterPortable);
    int rc = ensure_rows(pe, 0, T);
    if (prep.joinable()) prep.join();
    if (rc) return rc;
    if (pack && !him->p) return SHD_PE_ENOMEM;
    uint8_t* const hImg = static_cast<uint8_t*>(him->p);
    std::lock_guard<std::mutex> lk(pe->copyMu);
    const size_t G = pe->shards.size();
    std::vector<DevTemps> temps(G);
    std::vector<ShardFill> sf(G);
    for (size_t g = 0; g < G; ++g) {
        Shard* s = pe->shards[g].get();
        ShardFill& f = sf[g];
        f.s = s;
        f.pv = PackView{s->rowStart, s->rowStart + s->rowCount};
        temps[g].device = s->device;
        if (!s->rowCount) continue;
        if (!s->tableReady) return SHD_PE_ENOTOWNED;
        inf.shards++;
        HIPCHK(hipSetDevice(s->device));
        if (pack && packMode == 2 && (rc = ensure_pos_of(pe, s))) return rc;
        f.segBytes = off[(size_t)f.pv.hi] - off[(size_t)f.pv.lo];
        if (pack) {
            f.dImg = static_cast<uint8_t*>(temps[g].take(f.segBytes));
            f.dOff = static_cast<int64_t*>(temps[g].take((int64_t)off.size() * 8));
            f.dAcc = static_cast<unsigned long long*>(temps[g].take(16));
            f.dNeed = static_cast<int32_t*>(temps[g].take((int64_t)s->rowCount * 4));
        }
        f.dAll = static_cast<int32_t*>(temps[g].take((int64_t)s->rowCount * 4));
        if (!f.dAll || (pack && (!f.dImg || !f.dOff || !f.dAcc || !f.dNeed))) return SHD_PE_ENOMEM;
    }
    auto sync_all = [&]() -> int {
        for (ShardFill& f : sf) {
            if (!f.s->rowCount) continue;
            HIPCHK(hipSetDevice(f.s->device));
            HIPCHK(hipStreamSynchronize(f.s->copyStream));
        }
        return SHD_PE_OK;
    };
    // pack: every shard on its own device and copy stream
    const auto t1 = now();
    const unsigned long long acc0[2] = {0ull, 0x7FF0000000000000ull};
    for (ShardFill& f : sf) {
        Shard* s = f.s;
        if (!s->rowCount) continue;
        HIPCHK(hipSetDevice(s->device));
        if (pack) {
            HIPCHK(hipMemcpyAsync(f.dOff, off.data(), off.size() * 8, hipMemcpyHostToDevice, s->copyStream));
            HIPCHK(hipMemcpyAsync(f.dAcc, acc0, 16, hipMemcpyHostToDevice, s->copyStream));
            if (launch_pack_rowstore(s->tab, f.pv, f.dOff, f.dImg, f.dAcc, f.dNeed, packMode, &s->dgAux,
                                     s->dPosOf, wantDirect, pe->hg.isComplete, s->copyStream))
                return SHD_PE_ETOOBIG;
        }
        launch_rows_all_success(s->tab, s->rowCount, f.dAll, s->copyStream);
        HIPCHK(hipGetLastError());
    }
    if ((rc = sync_all())) return rc;
    // DMA: the segments to their place in the one image (distinct devices:
    // concurrently), then the small results
    const auto t2 = now();
    if (pack)
        for (ShardFill& f : sf) {
            if (!f.s->rowCount) continue;
            HIPCHK(hipSetDevice(f.s->device));
            HIPCHK(hipMemcpyAsync(hImg + off[(size_t)f.pv.lo], f.dImg, (size_t)f.segBytes, hipMemcpyDeviceToHost,
                                  f.s->copyStream));
        }
    for (ShardFill& f : sf) {
        Shard* s = f.s;
        if (!s->rowCount) continue;
        HIPCHK(hipSetDevice(s->device));
        if (pack) {
            f.needCount.resize((size_t)s->rowCount);
            HIPCHK(hipMemcpyAsync(f.acc, f.dAcc, 16, hipMemcpyDeviceToHost, s->copyStream));
            HIPCHK(hipMemcpyAsync(f.needCount.data(), f.dNeed, (size_t)s->rowCount * 4, hipMemcpyDeviceToHost,
                                  s->copyStream));
        }
        if (rowResult)
            HIPCHK(hipMemcpyAsync(rowResult + f.pv.lo, f.dAll, (size_t)s->rowCount * 4, hipMemcpyDeviceToHost,
                                  s->copyStream));
    }
    if ((rc = sync_all())) return rc;
    const auto t3 = now();
    // needs: lists in rounds, routed to the owners of their rows b, answered, applied
    FillTotals tot;
    int64_t maxRound = 0;
    for (ShardFill& f : sf) {
        if (f.needCount.empty()) continue;
        fill_plan_rounds(f.needCount.data(), (int32_t)f.needCount.size(), needBudgetBytes, f.rounds);
        for (size_t r = 0; r + 1 < f.rounds.size(); ++r) {
            int64_t n = 0;
            for (int32_t i = f.rounds[r]; i < f.rounds[r + 1]; ++i) n += f.needCount[(size_t)i];
            maxRound = std::max(maxRound, n);
            inf.needs += n;
        }
    }
    PinnedBlock stg;
    if (maxRound) {
        // pairs as listed | pairs by owner | lat | rel | ok
        if (hipHostMalloc(&stg.p, (size_t)maxRound * 33, hipHostMallocPortable) != hipSuccess) {
            stg.p = nullptr;
            return SHD_PE_ENOMEM;
        }
    }
    NeedPair* const hPairs = static_cast<NeedPair*>(stg.p);
    NeedPair* const hRouted = hPairs + maxRound;
    double* const hLat = reinterpret_cast<double*>(hRouted + maxRound);
    double* const hRel = hLat + maxRound;
    uint8_t* const hOk = reinterpret_cast<uint8_t*>(hRel + maxRound);
    std::vector<int32_t> rowsV;
    std::vector<int64_t> preV, start, order;
    std::vector<size_t> mark(G);
    for (size_t g = 0; g < G; ++g) {
        ShardFill& f = sf[g];
        Shard* s = f.s;
        for (size_t r = 0; r + 1 < f.rounds.size(); ++r) {
            rowsV.clear();
            preV.clear();
            int64_t n = 0;
            for (int32_t i = f.rounds[r]; i < f.rounds[r + 1]; ++i)
                if (f.needCount[(size_t)i] > 0) {
                    rowsV.push_back(f.pv.lo + i);
                    preV.push_back(n);
                    n += f.needCount[(size_t)i];
                }
            for (size_t o = 0; o < G; ++o) mark[o] = temps[o].blocks.size();
            const int32_t nr = (int32_t)rowsV.size();
            int32_t* dRows = static_cast<int32_t*>(temps[g].take((int64_t)nr * 4));
            int64_t* dPre = static_cast<int64_t*>(temps[g].take((int64_t)nr * 8));
            int32_t* dPairs = static_cast<int32_t*>(temps[g].take(n * 8));
            if (!dRows || !dPre || !dPairs) return SHD_PE_ENOMEM;
            HIPCHK(hipSetDevice(s->device));
            HIPCHK(hipMemcpyAsync(dRows, rowsV.data(), (size_t)nr * 4, hipMemcpyHostToDevice, s->copyStream));
            HIPCHK(hipMemcpyAsync(dPre, preV.data(), (size_t)nr * 8, hipMemcpyHostToDevice, s->copyStream));
            launch_pack_needs(f.pv, T, f.dOff, f.dImg, dRows, dPre, nr, dPairs, s->copyStream);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(hPairs, dPairs, (size_t)n * 8, hipMemcpyDeviceToHost, s->copyStream));
            HIPCHK(hipStreamSynchronize(s->copyStream));
            if (fill_route_needs(hPairs, n, pe->bounds.data(), (int32_t)G, start, order)) return SHD_PE_EHIP;
            for (int64_t j = 0; j < n; ++j) hRouted[j] = hPairs[order[(size_t)j]];
            for (size_t o = 0; o < G; ++o) {
                const int64_t at = start[o], c = start[o + 1] - at;
                if (!c) continue;
                Shard* ow = pe->shards[o].get();
                if (!ow->tableReady) return SHD_PE_ENOTOWNED;
                int32_t* dP = static_cast<int32_t*>(temps[o].take(c * 8));
                double* dLat = static_cast<double*>(temps[o].take(c * 8));
                double* dRel = static_cast<double*>(temps[o].take(c * 8));
                uint8_t* dOk = static_cast<uint8_t*>(temps[o].take(c));
                if (!dP || !dLat || !dRel || !dOk) return SHD_PE_ENOMEM;
                HIPCHK(hipSetDevice(ow->device));
                HIPCHK(hipMemcpyAsync(dP, hRouted + at, (size_t)c * 8, hipMemcpyHostToDevice, ow->copyStream));
                launch_pack_answer(ow->tab, dP, c, dOk, dLat, dRel, ow->copyStream);
                HIPCHK(hipGetLastError());
                HIPCHK(hipMemcpyAsync(hLat + at, dLat, (size_t)c * 8, hipMemcpyDeviceToHost, ow->copyStream));
                HIPCHK(hipMemcpyAsync(hRel + at, dRel, (size_t)c * 8, hipMemcpyDeviceToHost, ow->copyStream));
                HIPCHK(hipMemcpyAsync(hOk + at, dOk, (size_t)c, hipMemcpyDeviceToHost, ow->copyStream));
            }
            for (size_t o = 0; o < G; ++o) {
                if (start[o + 1] == start[o]) continue;
                HIPCHK(hipSetDevice(pe->shards[o]->device));
                HIPCHK(hipStreamSynchronize(pe->shards[o]->copyStream));
            }
            if (fill_apply_answers(hImg, off.data(), T, hRouted, n, hOk, hLat, hRel, packMode == 1, &tot))
                return SHD_PE_EHIP;   // a list that does not match the image's pending slots
            for (size_t o = 0; o < G; ++o) temps[o].release(mark[o]);
            inf.needRounds++;
        }
    }
    const auto t4 = now();
    inf.needsStored = tot.needsStored;
    for (size_t g = 0; g < G; ++g) inf.deviceBytesPeak = std::max(inf.deviceBytesPeak, temps[g].peak);
    if (pack) {
        int64_t stored = tot.stored;
        double mn = tot.minLatency;
        for (ShardFill& f : sf) {
            if (!f.s->rowCount) continue;
            double m;
            std::memcpy(&m, &f.acc[1], 8);
            stored += (int64_t)f.acc[0];
            mn = m < mn ? m : mn;
        }
        rc = shd_rowstore_adopt_image(st, hImg, (int64_t)bytes, host_image_free_cb, him.get(), stored, mn);
        if (rc) return rc;
        him.release();   // the store owns it now
    }
    inf.msCompute = ms(t0, t1);
    inf.msPack = ms(t1, t2);
    inf.msDma = ms(t2, t3);
    inf.msResolve = ms(t3, t4);
    if (info) *info = inf;
    return SHD_PE_OK;
}

// ---------------------------------------------------------------------------
// Gather: the whole table on every device of this engine (and, with a
// cross-process communicator, of every engine).
// ---------------------------------------------------------------------------
static int ensure_full(ShdPe* pe, Shard* s, Shard* owner) {
    if (s != owner) { s->full = owner->full; return SHD_PE_OK; }
    if (s->full.lat) return SHD_PE_OK;
    const size_t T = pe->attached.size();
    if (pe->G == 1) { s->full = s->tab; return SHD_PE_OK; }   // the shard is the table
    HIPCHK(hipSetDevice(s->device));
    return alloc_table(s, s->full, T, T, pe->opt.storePred != 0);
}

// The RCCL type that moves a field of this element size (bit patterns only).
static ncclDataType_t rccl_type(int esize) {
    return esize == 8 ? ncclUint64 : esize == 4 ? ncclInt32 : ncclUint8;
}

static int gather_locked(ShdPe* pe) {
    const int32_t T = (int32_t)pe->attached.size();
    std::vector<int32_t> all;
    for (int32_t p = pe->ownStart; p < pe->ownEnd; ++p)
        if (!row_done(pe, p)) all.push_back(p);
    int rc = compute_positions_locked(pe, all.data(), (int32_t)all.size());
    if (rc) return rc;
    for (auto& s : pe->shards) if ((rc = ensure_table(pe, s.get()))) return rc;
    // one full table per distinct device, owned by its first shard
    for (auto& s : pe->shards) {
        Shard* owner = nullptr;
        for (auto& o : pe->shards)
            if (o->device == s->device) { owner = o.get(); break; }
        if ((rc = ensure_full(pe, s.get(), owner))) return rc;
    }
    Shard* s0 = pe->shards[0].get();
    bool distinct = true;
    for (size_t i = 0; i < pe->shards.size(); ++i)
        for (size_t j = 0; j < i; ++j)
            if (pe->shards[i]->device == pe->shards[j]->device) distinct = false;
    // in-process RCCL over xGMI (distinct devices): one communicator per
    // device, created before the timed region
    if (pe->G > 1 && !pe->xcomm && distinct && !s0->comm) {
        std::vector<ncclComm_t> comms(pe->shards.size());
        std::vector<int> devs;
        for (auto& s : pe->shards) devs.push_back(s->device);
        if (ncclCommInitAll(comms.data(), (int)devs.size(), devs.data()) != ncclSuccess)
            return SHD_PE_ECOMM;
        for (size_t i = 0; i < comms.size(); ++i) pe->shards[i]->comm = comms[i];
    }
    struct Events {   // destroyed on every exit path
        hipEvent_t e[2] = {nullptr, nullptr};
        ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    } ev;
    HIPCHK(hipSetDevice(s0->device));
    HIPCHK(hipEventCreate(&ev.e[0]));
    HIPCHK(hipEventCreate(&ev.e[1]));
    hipEvent_t e0 = ev.e[0], e1 = ev.e[1];
    HIPCHK(hipEventRecord(e0, s0->stream));
    // rows [r0, r0 + nr), rank `root`'s shard, into their place in s's full
    // table; the root (isRoot) sends them from its own table
    auto bcast_rows = [&](Shard* s, bool isRoot, int root, ncclComm_t comm, int64_t r0, int64_t nr) {
        if (!nr) return;
        (void)for_each_field(isRoot ? s->tab : s->full, s->full, r0, nr,
                             [&](void* dst, const void* src, int64_t bytes, int esize) {
                                 if (ncclBroadcast(src, dst, (size_t)(bytes / esize), rccl_type(esize), root, comm,
                                                   s->stream) != ncclSuccess)
                                     rc = SHD_PE_ECOMM;
                                 return 0;
                             });
    };
    if (pe->G == 1 && !pe->xcomm) {
        // nothing to exchange
    } else if (pe->xcomm) {
        // cross-process: every process owns one shard (nDevices == 1), rows
        // contiguous per shard.  Equal blocks (the plan's usual outcome, e.g.
        // C4 over 8 ranks: 2,048 rows each): one ncclAllGather per field
        // straight into the full table; otherwise a group of per-shard
        // broadcasts (an all-gather-v with blocks landing in place)
        Shard* s = s0;
        bool equal = true;
        for (int g = 1; g < pe->G; ++g)
            equal = equal && pe->bounds[g + 1] - pe->bounds[g] == pe->bounds[1] - pe->bounds[0];
        if (ncclGroupStart() != ncclSuccess) return SHD_PE_ECOMM;
        if (equal) {
            // (the send view is the shard's rows re-based at 0: the receive
            // buffer of an all-gather is the table's start, rank g's block
            // landing g blocks into it)
            DevTable mine = s->tab;
            mine.rowStart = 0;
            (void)for_each_field(mine, s->full, 0, pe->bounds[1] - pe->bounds[0],
                                 [&](void* dst, const void* src, int64_t bytes, int esize) {
                                     if (bytes && ncclAllGather(src, dst, (size_t)(bytes / esize), rccl_type(esize),
                                                                pe->xcomm, s->stream) != ncclSuccess)
                                         rc = SHD_PE_ECOMM;
                                     return 0;
                                 });
        } else {
            for (int g = 0; g < pe->G && rc == SHD_PE_OK; ++g)
                bcast_rows(s, g == s->gindex, g, pe->xcomm, pe->bounds[g], pe->bounds[g + 1] - pe->bounds[g]);
        }
        if (ncclGroupEnd() != ncclSuccess) rc = SHD_PE_ECOMM;
        if (rc) return rc;
    } else {
        if (distinct) {
            // in-process RCCL over xGMI: a group of per-shard broadcasts
            if (ncclGroupStart() != ncclSuccess) return SHD_PE_ECOMM;
            for (size_t r = 0; r < pe->shards.size(); ++r) {
                Shard* root = pe->shards[r].get();
                for (auto& sp : pe->shards)
                    bcast_rows(sp.get(), sp.get() == root, (int)r, sp->comm, root->rowStart, root->rowCount);
            }
            if (ncclGroupEnd() != ncclSuccess) rc = SHD_PE_ECOMM;
            if (rc) return rc;
        } else {
            // logical shards sharing a device (tests): device / peer copies
            for (auto& src : pe->shards) {
                if (!src->rowCount) continue;
                for (auto& dstS : pe->shards) {
                    if (!dstS->fullOwner) continue;
                    HIPCHK(hipSetDevice(dstS->device));
                    if ((rc = for_each_field(src->tab, dstS->full, src->rowStart, src->rowCount,
                                             async_copy(hipMemcpyDeviceToDevice, dstS->stream))))
                        return rc;
                }
            }
        }
    }
    for (auto& s : pe->shards) {
        HIPCHK(hipSetDevice(s->device));
        HIPCHK(hipStreamSynchronize(s->stream));
    }
    HIPCHK(hipSetDevice(s0->device));
    HIPCHK(hipEventRecord(e1, s0->stream));
    HIPCHK(hipEventSynchronize(e1));
    pe->msGather += elapsed(e0, e1);
    for (int32_t p = 0; p < T; ++p) pe->rowDone[p].store(1, std::memory_order_release);
    pe->gathered = true;
    return SHD_PE_OK;
}

// Host-transport assembly (no RCCL): rows of other engines' shards arrive in
// host buffers (MPI, sockets, torch.distributed/gloo -- e.g. several ranks
// sharing one GPU, where RCCL refuses a communicator) and are written into
// the full table on every device of this engine; this engine's own rows are
// copied in on the first call.  Once all T rows are present the engine reads
// every row from the full table, as after shd_pe_gather.
extern "C" int shd_pe_put_rows(ShdPe* pe, int32_t start, int32_t count, const double* lat,
                               const double* rel, const int32_t* hops, const int32_t* pred,
                               const uint8_t* flags) {
    if (!pe || start < 0 || count < 0 || (int64_t)start + count > (int64_t)pe->attached.size())
        return SHD_PE_EINVAL;
    if (!lat || !rel || !hops || !flags || (pe->opt.storePred && !pred)) return SHD_PE_EINVAL;
    if (pe->opt.shardCount < 2 || pe->opt.nDevices != 1) return SHD_PE_EINVAL;
    if (start < pe->ownEnd && start + count > pe->ownStart) return SHD_PE_EINVAL;   // own rows
    if (count == 0) return SHD_PE_OK;
    std::lock_guard<std::mutex> lk(pe->mu);
    std::lock_guard<std::mutex> lk2(pe->copyMu);
    Shard* s = pe->shards[0].get();
    int rc = ensure_table(pe, s);
    if (rc) return rc;
    if (!pe->putInit) {
        std::vector<int32_t> all;
        for (int32_t p = pe->ownStart; p < pe->ownEnd; ++p)
            if (!row_done(pe, p)) all.push_back(p);
        if ((rc = compute_positions_locked(pe, all.data(), (int32_t)all.size()))) return rc;
        if ((rc = ensure_full(pe, s, s))) return rc;
        HIPCHK(hipSetDevice(s->device));
        if ((rc = for_each_field(s->tab, s->full, s->rowStart, s->rowCount,
                                 async_copy(hipMemcpyDeviceToDevice, s->stream))))
            return rc;
        HIPCHK(hipStreamSynchronize(s->stream));
        pe->putInit = true;
    }
    HIPCHK(hipSetDevice(s->device));
    const size_t ts = pe->attached.size();
    if ((rc = for_each_field(caller_view(lat, rel, hops, pred, flags, ts, start), s->full, start, count,
                             async_copy(hipMemcpyHostToDevice, s->stream))))
        return rc;
    HIPCHK(hipStreamSynchronize(s->stream));
    if (pe->putSeen.empty()) pe->putSeen.assign(ts, 0);
    for (int32_t p = start; p < start + count; ++p)
        if (!pe->putSeen[(size_t)p]) { pe->putSeen[(size_t)p] = 1; ++pe->putRows; }
    if (pe->putRows + (pe->ownEnd - pe->ownStart) >= (int64_t)ts) {
        for (size_t p = 0; p < ts; ++p) pe->rowDone[p].store(1, std::memory_order_release);
        pe->gathered = true;
    }
    return SHD_PE_OK;
}

extern "C" int shd_pe_gather(ShdPe* pe) {
    if (!pe) return SHD_PE_EINVAL;
    std::lock_guard<std::mutex> lk(pe->mu);
    std::lock_guard<std::mutex> lk2(pe->copyMu);
    if (pe->G > 1 && pe->opt.shardCount > 1 && !pe->xcomm) return SHD_PE_ECOMM;
    return gather_locked(pe);
}

extern "C" int shd_pe_comm_unique_id(void* out, int32_t bytes) {
    if (!out || bytes < (int32_t)sizeof(ncclUniqueId)) return SHD_PE_EINVAL;
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return SHD_PE_ECOMM;
    std::memcpy(out, &id, sizeof(id));
    return SHD_PE_OK;
}

extern "C" int shd_pe_comm_init(ShdPe* pe, const void* uniqueId, int32_t bytes) {
    if (!pe || !uniqueId || bytes < (int32_t)sizeof(ncclUniqueId)) return SHD_PE_EINVAL;
    // (shardCount 1: a one-rank communicator -- the gather then runs the same
    // RCCL calls as at N > 1, an in-place all-gather of the engine's own
    // rows: how the RCCL path is exercised on a one-GPU box)
    if (pe->opt.nDevices != 1 || pe->opt.shardCount < 1) return SHD_PE_EINVAL;
    std::lock_guard<std::mutex> lk(pe->mu);
    if (pe->xcomm) return SHD_PE_OK;
    ncclUniqueId id;
    std::memcpy(&id, uniqueId, sizeof(id));
    if (hipSetDevice(pe->shards[0]->device) != hipSuccess) return SHD_PE_EHIP;
    if (ncclCommInitRank(&pe->xcomm, pe->opt.shardCount, id, pe->opt.shardIndex) != ncclSuccess) {
        pe->xcomm = nullptr;
        return SHD_PE_ECOMM;
    }
    return SHD_PE_OK;
}

