// pe_fill.cpp -- host side of shd_pe_fill_rowstore_shards: need rounds,
// routing needs to the shards that own the rows, answers into the image.
// No HIP (pe_fill.hpp); the device half is k_pack_* in pe_aux.hip.
#include "pe_fill.hpp"

#include <algorithm>
#include <cstring>

#include "shd_pathengine.h"

namespace shdpe {

void fill_plan_rounds(const int32_t* needCount, int32_t nRows, int64_t budgetBytes,
                      std::vector<int32_t>& bounds) {
    bounds.clear();
    const int64_t budget = budgetBytes > 0 ? budgetBytes : FILL_NEED_BUDGET_DEFAULT;
    int32_t last = -1;                       // last row with needs
    for (int32_t r = 0; r < nRows; ++r)
        if (needCount[r] > 0) last = r;
    if (last < 0) return;
    bounds.push_back(0);
    int64_t cur = 0;                         // bytes of the open round
    for (int32_t r = 0; r <= last; ++r) {
        const int64_t b = (int64_t)needCount[r] * FILL_NEED_BYTES;
        if (cur > 0 && b > 0 && cur + b > budget) {
            bounds.push_back(r);
            cur = 0;
        }
        cur += b;
    }
    bounds.push_back(nRows);
}

int fill_route_needs(const NeedPair* needs, int64_t n, const int32_t* bounds, int32_t G,
                     std::vector<int64_t>& start, std::vector<int64_t>& order) {
    start.assign((size_t)G + 1, 0);
    order.assign((size_t)n, 0);
    std::vector<int32_t> owner((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const int32_t b = needs[i].b;
        if (b < bounds[0] || b >= bounds[G]) return -1;
        // the last g with bounds[g] <= b: an empty shard never owns a row
        const int32_t g = (int32_t)(std::upper_bound(bounds, bounds + G + 1, b) - bounds) - 1;
        owner[(size_t)i] = g;
        ++start[(size_t)g + 1];
    }
    for (int32_t g = 0; g < G; ++g) start[(size_t)g + 1] += start[(size_t)g];
    std::vector<int64_t> at(start.begin(), start.end() - 1);
    for (int64_t i = 0; i < n; ++i) order[(size_t)at[(size_t)owner[(size_t)i]]++] = i;
    return 0;
}

int fill_apply_answers(uint8_t* image, const int64_t* off, int32_t T, const NeedPair* needs, int64_t n,
                       const uint8_t* ok, const double* lat, const double* rel, bool completeDirect,
                       FillTotals* tot) {
    for (int64_t i = 0; i < n; ++i) {
        const int32_t a = needs[i].a, b = needs[i].b;
        if (a < 0 || b <= a || b >= T) return -1;
        const size_t len = (size_t)(T - a), k = (size_t)(b - a);
        uint8_t* row = image + off[a] + SHD_ROWSTORE_IMAGE_HEADER;
        uint8_t* S = row + len * 16;
        if (!(S[k] & FILL_S_PENDING)) return -1;
        uint8_t s = (uint8_t)(S[k] & ~FILL_S_PENDING);
        double l;
        if (ok[i]) {
            l = lat[i];
            std::memcpy(row + k * 8, &lat[i], 8);
            std::memcpy(row + len * 8 + k * 8, &rel[i], 8);
            s = (uint8_t)(SHD_ROWSTORE_S_STORED | SHD_ROWSTORE_S_REVERSED |
                          (completeDirect ? SHD_ROWSTORE_S_DIRECT : 0));
            ++tot->needsStored;
        } else {
            std::memcpy(&l, row + k * 8, 8);   // the provisional entry, if any
        }
        S[k] = s;
        if (s) {
            ++tot->stored;
            tot->minLatency = l < tot->minLatency ? l : tot->minLatency;
        }
    }
    return 0;
}

}  // namespace shdpe
