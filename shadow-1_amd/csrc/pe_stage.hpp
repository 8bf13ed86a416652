// pe_stage.hpp -- host <-> device copies of large pageable arrays through two
// page-locked staging buffers on one stream (shd_pe_graph_props' edge upload,
// the device graph build's upload and read-back).  Private to the library.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <thread>
#include <vector>

#include "shd_pathengine.h"

namespace shdpe {

constexpr size_t STAGE_BYTES = (size_t)16 << 20;        // an upload's chunk
constexpr size_t STAGE_DOWN_BYTES = (size_t)64 << 20;   // a download's chunk (fewer thread starts per byte)
constexpr size_t STAGE_COPY_THREADS = 8;

// Two staging buffers and their events; the buffers are made by the first
// copy that needs them (page-locking is a fixed cost a small call avoids) and
// released with the object.  The stream is the caller's.
struct Stager {
    hipStream_t stream = nullptr;
    void* buf[2] = {nullptr, nullptr};
    size_t cap = 0;                          // bytes of each buffer made so far
    hipEvent_t ev[2] = {nullptr, nullptr};

    ~Stager() {
        for (void* p : buf)
            if (p) (void)hipHostFree(p);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }

    // buffers 0 .. count-1 of at least `bytes` bytes (a larger request than
    // the first replaces the buffers once their copies have drained)
    int ensure(int count, size_t bytes) {
        if (bytes > cap) {
            if (cap && hipStreamSynchronize(stream) != hipSuccess) return SHD_PE_EHIP;
            for (void*& p : buf)
                if (p) { (void)hipHostFree(p); p = nullptr; }
            cap = bytes;
        }
        for (int b = 0; b < count; ++b) {
            if (!buf[b] && hipHostMalloc(&buf[b], cap) != hipSuccess) {
                buf[b] = nullptr;
                return SHD_PE_ENOMEM;
            }
            if (!ev[b] && hipEventCreateWithFlags(&ev[b], hipEventDisableTiming) != hipSuccess) {
                ev[b] = nullptr;
                return SHD_PE_EHIP;
            }
        }
        return SHD_PE_OK;
    }

    // Host array -> device, asynchronous on the stream: a page-locked source
    // goes by DMA directly, a pageable one in chunks through the buffers.
    int upload(void* dst, const void* src, size_t bytes) {
        if (bytes == 0) return SHD_PE_OK;
        hipPointerAttribute_t attr;
        const bool locked = hipPointerGetAttributes(&attr, src) == hipSuccess && attr.type == hipMemoryTypeHost;
        (void)hipGetLastError();               // an unregistered pointer may report an error: not one of ours
        if (locked)
            return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream) == hipSuccess ? SHD_PE_OK
                                                                                                 : SHD_PE_EHIP;
        // a second buffer only where there is a second chunk
        const size_t chunk = std::min(STAGE_BYTES, bytes);
        const bool two = bytes > chunk;
        const int rc = ensure(two ? 2 : 1, chunk);
        if (rc) return rc;
        int b = 0;
        for (size_t off = 0; off < bytes; off += chunk, b = two ? b ^ 1 : 0) {
            const size_t len = std::min(chunk, bytes - off);
            if (hipEventSynchronize(ev[b]) != hipSuccess) return SHD_PE_EHIP;   // the buffer's previous DMA (done at once if none)
            std::memcpy(buf[b], (const char*)src + off, len);
            if (hipMemcpyAsync((char*)dst + off, buf[b], len, hipMemcpyHostToDevice, stream) != hipSuccess ||
                hipEventRecord(ev[b], stream) != hipSuccess)
                return SHD_PE_EHIP;
        }
        return SHD_PE_OK;
    }

    // Out of a staging buffer into pageable memory the caller has not touched
    // yet: the copy is page faults as much as bytes, so a large one is split
    // over a few threads.
    static void copy_out(char* dst, const char* src, size_t len) {
        constexpr size_t PER_THREAD = (size_t)4 << 20;
        const int nt = (int)std::min<size_t>(STAGE_COPY_THREADS, len / PER_THREAD);
        if (len == 0) return;
        if (nt <= 1) { std::memcpy(dst, src, len); return; }
        std::vector<std::thread> th;
        auto part = [&](int t) {
            const size_t lo = len * (size_t)t / (size_t)nt, hi = len * (size_t)(t + 1) / (size_t)nt;
            std::memcpy(dst + lo, src + lo, hi - lo);
        };
        for (int t = 1; t < nt; ++t) th.emplace_back(part, t);
        part(0);
        for (auto& x : th) x.join();
    }

    // Device array -> pageable host array, complete on return: the DMA of one
    // chunk runs while the previous one is copied out of its buffer.
    int download(void* dst, const void* src, size_t bytes) {
        if (bytes == 0) return SHD_PE_OK;
        const size_t chunk = std::min(STAGE_DOWN_BYTES, bytes);
        const bool two = bytes > chunk;
        const int rc = ensure(two ? 2 : 1, chunk);
        if (rc) return rc;
        // (an upload may still own a buffer)
        if (hipStreamSynchronize(stream) != hipSuccess) return SHD_PE_EHIP;
        auto start = [&](size_t off, int b) {
            const size_t len = std::min(chunk, bytes - off);
            return hipMemcpyAsync(buf[b], (const char*)src + off, len, hipMemcpyDeviceToHost, stream) == hipSuccess &&
                   hipEventRecord(ev[b], stream) == hipSuccess;
        };
        if (!start(0, 0)) return SHD_PE_EHIP;
        int b = 0;
        for (size_t off = 0; off < bytes; off += chunk, b ^= 1) {
            const size_t next = off + chunk;
            if (next < bytes && !start(next, b ^ 1)) return SHD_PE_EHIP;
            if (hipEventSynchronize(ev[b]) != hipSuccess) return SHD_PE_EHIP;
            copy_out((char*)dst + off, (const char*)buf[b], std::min(chunk, bytes - off));
        }
        return SHD_PE_OK;
    }
};

}  // namespace shdpe
