// pe_fill.hpp -- the host half of the shard-by-shard path-cache fill
// (shd_pe_fill_rowstore_shards, pe_rows.hip): what happens to the needs the
// pack kernel leaves behind.  Free functions over plain arrays, no HIP and no
// engine state (like pe_plan.hpp), so they build and test without a device.
#pragma once
#include <stdint.h>

#include <vector>

namespace shdpe {

// The pack kernel's PACK_S_PENDING (pe_device.hpp), restated for host code
// that includes no device header.
constexpr uint8_t FILL_S_PENDING = 0x80;
// One need in flight: its (a, b) pair out, ok / lat / rel back.
constexpr int64_t FILL_NEED_BYTES = 8 + 1 + 8 + 8;
constexpr int64_t FILL_NEED_BUDGET_DEFAULT = (int64_t)64 << 20;

struct NeedPair {
    int32_t a, b;   // table positions, a < b: slot b - a of image row a wants entry (b, a)
};

// Rounds over a view's rows: bounds[i] .. bounds[i + 1] are the local rows of
// round i, consecutive ranges whose needs times FILL_NEED_BYTES stay within
// budgetBytes (<= 0: the default); a single row past the budget gets a round
// to itself.  Rows without needs ride along; no round is empty of needs, and
// there is none when no row has any.
void fill_plan_rounds(const int32_t* needCount, int32_t nRows, int64_t budgetBytes,
                      std::vector<int32_t>& bounds);

// Needs by the shard that owns row b (bounds: G + 1 ascending positions, empty
// shards allowed): order[start[g] .. start[g + 1]) are the indices of owner
// g's needs, in list order.  -1: a row b outside [bounds[0], bounds[G]).
int fill_route_needs(const NeedPair* needs, int64_t n, const int32_t* bounds, int32_t G,
                     std::vector<int64_t>& start, std::vector<int64_t>& order);

struct FillTotals {
    int64_t stored = 0;        // slots whose final state is non-zero (for the count)
    int64_t needsStored = 0;   // of the needs, answered ok
    double minLatency = 1.0 / 0.0;
};

// Answers into the landed image (off: shd_rowstore_image_layout of T).  ok:
// the slot becomes the reverse entry -- lat, rel, STORED | REVERSED, and
// DIRECT when completeDirect (a complete graph's direct table); otherwise it
// keeps what the pack left (a direct entry or nothing).  Either way PENDING
// goes, and a slot that ends non-empty is added to tot.  -1: a pair outside
// the image or a slot that was not pending (nothing further is applied).
int fill_apply_answers(uint8_t* image, const int64_t* off, int32_t T, const NeedPair* needs, int64_t n,
                       const uint8_t* ok, const double* lat, const double* rel, bool completeDirect,
                       FillTotals* tot);

}  // namespace shdpe
