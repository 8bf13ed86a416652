// pe_build.hpp -- the engine's graph built on the device (pe_build.hip): from
// the caller's edge list straight to the arrays of DevGraph, HostGraph read
// back from them.  Private to the library.
#pragma once
#include <stdint.h>

#include <vector>

#include "pe_device.hpp"
#include "pe_graph.hpp"
#include "shd_pathengine.h"

namespace shdpe {

// The row kernel keeps an n-bit neighbour bitmap and a prefix count per
// bitmap word in LDS: 8 B per 32 vertices, 32 KiB at this vertex count.
// Graphs past it are built by the host form (handOffWhy 2).
constexpr int32_t BUILD_MAX_N = 131072;

// SHD_PE_BUILD_AUTO: the edge count from which the device build is chosen: the
// smallest complete graph measured (n = 2,500) at and past which the device
// build's median create time beats the host build's by more than the
// run-to-run spread (profiles/create_device_build.json, "auto_threshold_edges";
// DESIGN.md 8e).  At n = 1,000 (500,500 edges) the two are level.
constexpr int64_t BUILD_AUTO_MIN_EDGES = 3126250;

// What the device build leaves on its device: the graph arrays of DevGraph
// that do not depend on the attached list or the kernel configuration
// (attached, isAttached and heavyBits are made by finish_built_graph once a
// shard is configured).  Whoever adopts it takes `allocs`; otherwise they are
// freed with the object.
struct BuiltGraph {
    int device = -1;
    DevGraph dg{};
    std::vector<void*> allocs;
    bool adopted = false;
    void release();                 // frees what nobody adopted
    ~BuiltGraph();
};

// Build on `device` (a gfx950, already checked).  SHD_PE_OK with
// info->handedOff = 0: *g and *out hold the graph.  SHD_PE_OK with
// info->handedOff = 1 (handOffWhy set): nothing was built, the caller runs
// build_host_graph.  Fills info's msUpload / msKernels / msReadback /
// deviceBytesPeak.
int device_build_graph(const ShdPeGraphDesc* d, int device, int32_t maxN, HostGraph* g, BuiltGraph* out,
                       ShdPeBuildInfo* info);

// attached / isAttached / heavyBits of a built graph, on `stream` of the
// built graph's device (the current one); the arrays go into `allocs`.
int finish_built_graph(const std::vector<int32_t>& attached, int32_t heavyDeg, void* stream, DevGraph* dg,
                       std::vector<void*>* allocs);

// One digest per array (shd_pe_graph_digest): `count` elements of `width`
// bytes (1, 4 or 8) at device pointer `p`, zero-extended; *out receives the
// wrapping sum of splitmix64(bits ^ index * 0x9e3779b97f4a7c15).  dAcc is a
// device u64 the caller owns.  Synchronous.
int device_array_digest(const void* p, int width, int64_t count, uint64_t* dAcc, void* stream, uint64_t* out);
uint64_t host_array_digest(const void* p, int width, int64_t count);

}  // namespace shdpe
