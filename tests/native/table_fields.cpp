// The table-field walk of pe_device.hpp (TABLE_FIELDS, for_each_field,
// stage_view) over small host arrays with memcpy as the copy: which bytes a
// transfer between two DevTable views moves, and that it touches no others.
// Built with -fsanitize=address,undefined by tests/test_host.py; no HIP.
#include <cstdio>
#include <cstring>
#include <vector>

#include "pe_device.hpp"

using namespace shdpe;

namespace {

constexpr int64_t T = 7;
constexpr unsigned char FILL = 0xA5;
constexpr unsigned LAT = 1, REL = 2, HOPS = 4, PRED = 8, FLAGS = 16, ALL = 31;   // bit i: TABLE_FIELDS[i]

static_assert(sizeof(TABLE_FIELDS) / sizeof(TABLE_FIELDS[0]) == 5, "five fields");
static_assert(table_cell_bytes() == 8 + 8 + 4 + 4 + 1, "bytes per table cell");

int failures = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } \
    } while (0)

// Byte k of field fi's cell (pos, col) of the table: never FILL.
unsigned char cell_byte(int fi, int64_t pos, int64_t col, int k) {
    return (unsigned char)(1 + (fi * 53 + pos * 29 + col * 11 + k * 7) % 0xA0);
}

// Rows [rowStart, rowStart + rows) of every field, on the heap (the sanitizer sees a byte past either end).
struct Mem {
    int64_t rowStart, rows;
    std::vector<unsigned char> f[5];
    Mem(int64_t rs, int64_t n, bool table) : rowStart(rs), rows(n) {
        for (int fi = 0; fi < 5; ++fi) {
            const int es = TABLE_FIELDS[fi].esize;
            f[fi].assign((size_t)(rows * T * es), FILL);
            if (!table) continue;
            for (int64_t r = 0; r < rows; ++r)
                for (int64_t c = 0; c < T; ++c)
                    for (int k = 0; k < es; ++k) f[fi][(size_t)((r * T + c) * es + k)] = cell_byte(fi, rs + r, c, k);
        }
    }
    DevTable view(unsigned mask = ALL) {
        DevTable v{};
        v.T = T;
        v.rowStart = rowStart;
        for (int fi = 0; fi < 5; ++fi)
            if (mask >> fi & 1) set_table_field(v, TABLE_FIELDS[fi], f[fi].data());
        return v;
    }
    // fields of `mask`, rows [r0, r0 + n): the table's bytes; everything else: still FILL
    bool holds(unsigned mask, int64_t r0, int64_t n) const {
        for (int fi = 0; fi < 5; ++fi) {
            const int es = TABLE_FIELDS[fi].esize;
            for (int64_t r = 0; r < rows; ++r)
                for (int64_t c = 0; c < T; ++c)
                    for (int k = 0; k < es; ++k) {
                        const int64_t pos = rowStart + r;
                        const bool copied = (mask >> fi & 1) && pos >= r0 && pos < r0 + n;
                        if (f[fi][(size_t)((r * T + c) * es + k)] != (copied ? cell_byte(fi, pos, c, k) : FILL))
                            return false;
                    }
        }
        return true;
    }
};

int copy_bytes(void* dst, const void* src, int64_t bytes, int) {
    std::memcpy(dst, src, (size_t)bytes);
    return 0;
}

void test_views() {
    Mem shard(3, 6, true);                       // rows 3..8 of 11
    CHECK(shard.holds(ALL, 3, 6));
    {   // all five fields, the rows both views hold
        Mem out(4, 6, false);
        CHECK(for_each_field(shard.view(), out.view(), 4, 5, copy_bytes) == 0);
        CHECK(out.holds(ALL, 4, 5));
    }
    for (int fi = 0; fi < 5; ++fi) {             // each single field, on either side
        Mem a(4, 6, false), b(4, 6, false);
        CHECK(for_each_field(shard.view(), a.view(1u << fi), 4, 5, copy_bytes) == 0);
        CHECK(a.holds(1u << fi, 4, 5));
        CHECK(for_each_field(shard.view(1u << fi), b.view(), 4, 5, copy_bytes) == 0);
        CHECK(b.holds(1u << fi, 4, 5));
    }
    {   // no predecessors on the source only, on the destination only
        Mem a(4, 6, false), b(4, 6, false);
        CHECK(for_each_field(shard.view(ALL & ~PRED), a.view(), 4, 5, copy_bytes) == 0);
        CHECK(a.holds(ALL & ~PRED, 4, 5));
        CHECK(for_each_field(shard.view(), b.view(ALL & ~PRED), 4, 5, copy_bytes) == 0);
        CHECK(b.holds(ALL & ~PRED, 4, 5));
    }
    {   // a strict sub-range of both views
        Mem out(4, 6, false);
        CHECK(for_each_field(shard.view(), out.view(), 5, 3, copy_bytes) == 0);
        CHECK(out.holds(ALL, 5, 3));
    }
    {   // the copy's failure ends the walk and is returned
        Mem out(4, 6, false);
        int calls = 0;
        CHECK(for_each_field(shard.view(), out.view(), 4, 5, [&](void*, const void*, int64_t, int) {
                  ++calls;
                  return calls == 2 ? -7 : 0;
              }) == -7);
        CHECK(calls == 2);
        CHECK(out.holds(0, 0, 0));
    }
    {   // the element size handed to the copy, in the fields' order
        Mem out(4, 6, false);
        std::vector<int> es;
        std::vector<int64_t> by;
        (void)for_each_field(shard.view(), out.view(), 4, 5, [&](void*, const void*, int64_t bytes, int e) {
            es.push_back(e);
            by.push_back(bytes);
            return 0;
        });
        CHECK((es == std::vector<int>{8, 8, 4, 4, 1}));
        CHECK((by == std::vector<int64_t>{5 * T * 8, 5 * T * 8, 5 * T * 4, 5 * T * 4, 5 * T}));
    }
}

// table -> staging block -> caller, {lat, flags} only, rows 4..8 in blocks of 3 (3 + 2)
void test_staging() {
    Mem shard(3, 6, true), out(4, 6, false);
    const unsigned want = LAT | FLAGS;
    const DevTable caller = out.view(want);
    const int64_t B = 3, r0 = 4, n = 5;
    const size_t stageBytes = (size_t)(B * T * table_cell_bytes());   // sized by the full row, as the engine's
    std::vector<unsigned char> stage[2] = {std::vector<unsigned char>(stageBytes, FILL),
                                           std::vector<unsigned char>(stageBytes, FILL)};
    int buf = 0;
    for (int64_t b0 = r0; b0 < r0 + n; b0 += B, buf ^= 1) {
        const int64_t bn = b0 + B <= r0 + n ? B : r0 + n - b0;
        const DevTable sv = stage_view(stage[buf].data(), b0, bn, caller);
        CHECK(sv.rel == nullptr && sv.hops == nullptr && sv.pred == nullptr);
        CHECK((unsigned char*)sv.lat == stage[buf].data());
        CHECK(sv.flags == stage[buf].data() + bn * T * 8);           // packed back to back
        CHECK(for_each_field(shard.view(), sv, b0, bn, copy_bytes) == 0);         // issue
        // the block: bn rows of lat, bn rows of flags, the rest untouched
        size_t q = 0;
        bool ok = true;
        for (int fi : {0, 4})
            for (int64_t r = 0; r < bn; ++r)
                for (int64_t c = 0; c < T; ++c)
                    for (int k = 0; k < TABLE_FIELDS[fi].esize; ++k)
                        ok = ok && stage[buf][q++] == cell_byte(fi, b0 + r, c, k);
        CHECK(q == (size_t)(bn * T * 9));
        for (; q < stageBytes; ++q) ok = ok && stage[buf][q] == FILL;
        CHECK(ok);
        CHECK(for_each_field(sv, caller, b0, bn, copy_bytes) == 0);               // drain
        CHECK(out.holds(want, r0, b0 + bn - r0));
    }
    CHECK(buf == 0);                             // two blocks
    CHECK(out.holds(want, r0, n));
}

}  // namespace

int main() {
    test_views();
    test_staging();
    if (failures) return 1;
    std::printf("OK\n");
    return 0;
}
