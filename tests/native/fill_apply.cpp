// Host half of shd_pe_fill_rowstore_shards (pe_fill.cpp) with the row store
// (pe_rowstore.cpp), stand-alone: images as the pack kernel leaves them for a
// set of row shards -- hand-made pending slots, with and without a provisional
// direct entry -- get their needs planned into rounds, routed to owners,
// answered (ok and failed) and applied; the adopted store must equal a plain
// loop of shd_rowstore_store calls on every get, size and minimum latency.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "pe_fill.hpp"
#include "shd_pathengine.h"

using namespace shdpe;

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);      \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

static void release_image(void*, void* image) { std::free(image); }

struct Slot {          // what the finished store must hold for pair (a, a + k)
    uint8_t state = 0; // SHD_ROWSTORE_S_* bits, 0 empty
    double lat = 0, rel = 0;
};

static int owner_of(const std::vector<int32_t>& bounds, int32_t p) {
    for (size_t g = 0; g + 1 < bounds.size(); ++g)
        if (p >= bounds[g] && p < bounds[g + 1]) return (int)g;
    return -1;
}

// One table size, one shard plan, one mode and one budget.
// budget == FILL_NEED_BYTES: no image row gets a second need, so every round
// must hold exactly one.
static long run_case(int32_t T, const std::vector<int32_t>& bounds, bool completeDirect, int64_t budget,
                     unsigned seed) {
    const bool oneNeedPerRow = budget == FILL_NEED_BYTES;
    const int32_t G = (int32_t)bounds.size() - 1, n = 2 * T + 3;
    std::mt19937 rng(seed);
    auto coin = [&](int k) { return (int)(rng() % (unsigned)k); };
    auto value = [&] { return 1.0 + (double)(rng() % 100000) / 7.0; };
    std::vector<int32_t> att((size_t)T);
    for (int32_t j = 0; j < T; ++j) att[(size_t)j] = (j % 2 ? n - 1 - j : j + 1);   // distinct, not in id order
    std::vector<int64_t> off((size_t)T + 1);
    CHECK(shd_rowstore_image_layout(T, off.data()) == 0);
    uint8_t* img = static_cast<uint8_t*>(std::aligned_alloc(64, (size_t)std::max<int64_t>(off[(size_t)T], 64)));
    CHECK(img);
    std::memset(img, 0, (size_t)std::max<int64_t>(off[(size_t)T], 64));

    std::vector<std::vector<Slot>> want((size_t)T);
    std::vector<NeedPair> needs;                        // in the order the lists hold them
    std::vector<uint8_t> ansOk;
    std::vector<double> ansLat, ansRel;
    std::vector<std::vector<int32_t>> needCount((size_t)G);
    int64_t packStored = 0;                             // what the pack kernels' accumulators hold
    double packMin = INFINITY;
    long nOkPlain = 0, nOkProv = 0, nFailPlain = 0, nFailProv = 0;
    for (int32_t g = 0; g < G; ++g) needCount[(size_t)g].assign((size_t)(bounds[(size_t)g + 1] - bounds[(size_t)g]), 0);
    for (int32_t a = 0; a < T; ++a) {
        const int g = owner_of(bounds, a);
        CHECK(g >= 0);
        const int32_t hi = bounds[(size_t)g + 1], len = T - a;
        double* L = reinterpret_cast<double*>(img + off[(size_t)a] + SHD_ROWSTORE_IMAGE_HEADER);
        double* R = L + len;
        uint8_t* S = reinterpret_cast<uint8_t*>(R + len);
        want[(size_t)a].resize((size_t)len);
        for (int32_t k = 0; k < len; ++k) {
            const int32_t b = a + k;
            Slot w;
            const uint8_t dir = completeDirect ? SHD_ROWSTORE_S_DIRECT : 0;
            const bool full = oneNeedPerRow && needCount[(size_t)g][(size_t)(a - bounds[(size_t)g])] > 0;
            const int kind = coin(k > 0 && b >= hi && !full ? 6 : 4);
            if (kind == 0) {                            // forward entry
                w = Slot{(uint8_t)(SHD_ROWSTORE_S_STORED | dir), value(), value()};
            } else if (kind == 1) {                     // nothing, and no need (forward failed at k == 0, ...)
            } else if (kind == 2) {                     // a direct entry the pack decided alone
                w = Slot{(uint8_t)(SHD_ROWSTORE_S_STORED | SHD_ROWSTORE_S_DIRECT |
                                   (k > 0 && coin(2) ? SHD_ROWSTORE_S_REVERSED : 0)), value(), value()};
            } else if (kind == 3) {                     // the reverse entry from the shard's own rows
                if (k > 0 && b < hi)
                    w = Slot{(uint8_t)(SHD_ROWSTORE_S_STORED | SHD_ROWSTORE_S_REVERSED | dir), value(), value()};
            }
            if (kind <= 3) {
                L[k] = w.lat;
                R[k] = w.rel;
                S[k] = w.state;
                if (w.state) { ++packStored; packMin = std::min(packMin, w.lat); }
            } else {                                    // a need, kind 5 with a provisional direct entry
                const bool prov = kind == 5 && !completeDirect, ok = coin(2) != 0;
                Slot p;
                if (prov) p = Slot{(uint8_t)(SHD_ROWSTORE_S_STORED | SHD_ROWSTORE_S_DIRECT), value(), value()};
                L[k] = p.lat;
                R[k] = p.rel;
                S[k] = (uint8_t)(p.state | FILL_S_PENDING);
                const double al = value(), ar = value();
                needs.push_back(NeedPair{a, b});
                ansOk.push_back(ok ? 1 : 0);
                ansLat.push_back(al);
                ansRel.push_back(ar);
                needCount[(size_t)g][(size_t)(a - bounds[(size_t)g])]++;
                w = ok ? Slot{(uint8_t)(SHD_ROWSTORE_S_STORED | SHD_ROWSTORE_S_REVERSED | dir), al, ar} : p;
                (ok ? (prov ? nOkProv : nOkPlain) : (prov ? nFailProv : nFailPlain))++;
            }
            want[(size_t)a][(size_t)k] = w;
        }
    }

    // rounds per shard, lists per round, routing, answers in routed order, apply
    FillTotals tot;
    int64_t at = 0, rounds = 0;
    for (int32_t g = 0; g < G; ++g) {
        std::vector<int32_t> rb;
        const std::vector<int32_t>& nc = needCount[(size_t)g];
        fill_plan_rounds(nc.data(), (int32_t)nc.size(), budget, rb);
        int64_t shardNeeds = 0;
        for (int32_t c : nc) shardNeeds += c;
        CHECK(rb.empty() == (shardNeeds == 0));
        if (!rb.empty()) CHECK(rb.front() == 0 && rb.back() == (int32_t)nc.size());
        for (size_t r = 0; r + 1 < rb.size(); ++r) {
            CHECK(rb[r] < rb[r + 1]);
            int64_t cnt = 0, rowsWith = 0;
            for (int32_t i = rb[r]; i < rb[r + 1]; ++i) { cnt += nc[(size_t)i]; rowsWith += nc[(size_t)i] > 0; }
            CHECK(cnt > 0);
            const int64_t lim = budget > 0 ? budget : FILL_NEED_BUDGET_DEFAULT;
            CHECK(cnt * FILL_NEED_BYTES <= lim || rowsWith == 1);
            const NeedPair* list = needs.data() + at;
            std::vector<int64_t> start, order;
            CHECK(fill_route_needs(list, cnt, bounds.data(), G, start, order) == 0);
            CHECK((int32_t)start.size() == G + 1 && start[0] == 0 && start[(size_t)G] == cnt);
            std::vector<NeedPair> routed((size_t)cnt);
            std::vector<uint8_t> ok((size_t)cnt);
            std::vector<double> lat((size_t)cnt), rel((size_t)cnt);
            std::vector<uint8_t> seen((size_t)cnt, 0);
            for (int32_t o = 0; o < G; ++o)
                for (int64_t j = start[(size_t)o]; j < start[(size_t)o + 1]; ++j) {
                    const int64_t i = order[(size_t)j];
                    CHECK(i >= 0 && i < cnt && !seen[(size_t)i]);
                    seen[(size_t)i] = 1;
                    CHECK(owner_of(bounds, list[i].b) == o && o > g);      // another shard's row, behind this one
                    if (j > start[(size_t)o]) CHECK(order[(size_t)j - 1] < i);   // list order kept
                    routed[(size_t)j] = list[i];
                    ok[(size_t)j] = ansOk[(size_t)(at + i)];
                    lat[(size_t)j] = ansLat[(size_t)(at + i)];
                    rel[(size_t)j] = ansRel[(size_t)(at + i)];
                }
            CHECK(fill_apply_answers(img, off.data(), T, routed.data(), cnt, ok.data(), lat.data(), rel.data(),
                                     completeDirect, &tot) == 0);
            // a second application finds no pending slot
            FillTotals again;
            CHECK(fill_apply_answers(img, off.data(), T, routed.data(), 1, ok.data(), lat.data(), rel.data(),
                                     completeDirect, &again) == -1);
            at += cnt;
            ++rounds;
        }
    }
    CHECK(at == (int64_t)needs.size());
    if (oneNeedPerRow) CHECK(rounds == (int64_t)needs.size());
    CHECK(tot.needsStored == nOkPlain + nOkProv);
    CHECK(tot.stored == nOkPlain + nOkProv + nFailProv);
    const NeedPair outside{0, T};
    std::vector<int64_t> s2, o2;
    CHECK(fill_route_needs(&outside, 1, bounds.data(), G, s2, o2) == -1);

    // the reference: plain stores of the finished slots, in slot order
    ShdRowStore *ref = nullptr, *st = nullptr;
    CHECK(shd_rowstore_new(n, att.data(), T, &ref) == 0 && shd_rowstore_new(n, att.data(), T, &st) == 0);
    for (int32_t a = 0; a < T; ++a)
        for (int32_t k = 0; a + k < T; ++k) {
            const Slot& w = want[(size_t)a][(size_t)k];
            const uint8_t* S = img + off[(size_t)a] + SHD_ROWSTORE_IMAGE_HEADER + (size_t)(T - a) * 16;
            CHECK(!(S[k] & FILL_S_PENDING) && S[k] == w.state);
            if (!w.state) continue;
            const bool rev = (w.state & SHD_ROWSTORE_S_REVERSED) != 0;
            const int isd = (w.state & SHD_ROWSTORE_S_DIRECT) ? 1 : 0;
            CHECK(shd_rowstore_store(ref, att[(size_t)(rev ? a + k : a)], att[(size_t)(rev ? a : a + k)], isd, 0, 0,
                                     w.lat, w.rel) == 1);
        }
    const double mn = std::min(packMin, tot.minLatency);
    CHECK(shd_rowstore_adopt_image(st, img, off[(size_t)T], release_image, nullptr, packStored + tot.stored, mn) == 0);
    CHECK(shd_rowstore_size(st) == shd_rowstore_size(ref));
    CHECK(shd_rowstore_min_latency(st) == shd_rowstore_min_latency(ref));
    for (int32_t s = 0; s < n; ++s)
        for (int32_t d = 0; d < n; ++d) {
            double l1 = -1, r1 = -1, l2 = -1, r2 = -1;
            int32_t d1 = -1, d2 = -1;
            const int h1 = shd_rowstore_get(st, s, d, &l1, &r1, &d1, nullptr);
            const int h2 = shd_rowstore_get(ref, s, d, &l2, &r2, &d2, nullptr);
            CHECK(h1 == h2 && l1 == l2 && r1 == r2 && d1 == d2);
        }
    shd_rowstore_free(st);     // frees the image
    shd_rowstore_free(ref);
    if (T > 1 && G > 1 && bounds[1] > 0 && bounds[1] < T) CHECK(!needs.empty());
    if (T == 65 && !oneNeedPerRow && G > 1 && bounds[1] > 2 && bounds[1] < T - 2)
        CHECK(nOkPlain && nFailPlain && (completeDirect || (nOkProv && nFailProv)));
    return (long)needs.size();
}

int main() {
    long cases = 0, needs = 0;
    unsigned seed = 1;
    for (int32_t T : {1, 17, 65}) {
        std::vector<std::vector<int32_t>> plans = {
            {0, T},                                   // one owner: no needs
            {0, T / 2, T},                            // two
            {0, 0, T / 3, T / 3, T},                  // four, two of them empty
            {0, T / 4, T / 2, T},                     // three
            {0, T / 4, T / 2, (3 * T) / 4, T},        // four
            {0, T, T, T},                             // everything in the first of three
        };
        for (const auto& b : plans)
            for (int mode = 0; mode < 2; ++mode)
                for (int64_t budget : {(int64_t)0, FILL_NEED_BYTES, (int64_t)1, (int64_t)(3 * FILL_NEED_BYTES)}) {
                    needs += run_case(T, b, mode == 1, budget, seed++);
                    ++cases;
                }
    }
    // rounds: a row past the budget alone, rows without needs riding along
    {
        const int32_t nc[8] = {0, 2, 0, 9, 1, 0, 1, 0};
        std::vector<int32_t> rb;
        fill_plan_rounds(nc, 8, 3 * FILL_NEED_BYTES, rb);
        const std::vector<int32_t> expect = {0, 3, 4, 8};
        CHECK(rb == expect);
        fill_plan_rounds(nc, 8, 0, rb);
        CHECK((rb == std::vector<int32_t>{0, 8}));
        const int32_t none[3] = {0, 0, 0};
        fill_plan_rounds(none, 3, 1, rb);
        CHECK(rb.empty());
        fill_plan_rounds(none, 0, 1, rb);
        CHECK(rb.empty());
    }
    std::printf("OK %ld cases %ld needs\n", cases, needs);
    return 0;
}
