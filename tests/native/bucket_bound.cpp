// bucket_bound of pe_bucket.hpp (the delta-stepping bucket bound of both relax
// kernels) on the host, over random and adversarial (mn, delta) with finite
// mn >= 0 and delta > 0.  Built alone with -fsanitize=address,undefined; no HIP.
//
//   bucket_bound    every check, then "OK" when all hold
//
// The properties:
//   strict   the bound is strictly above mn (a relax loop that raises its bound
//            to it retires the minimum key: it cannot spin);
//   parent   wherever the formula the kernels had before the header (restated
//            in parent_bound below) is strictly above mn, the bound is that,
//            bit for bit (tables do not change);
//   inf      delta = +inf gives +inf (one bucket);
//   sweep    raising the bound over a sorted list of n keys the way the kernels
//            do reaches the end in at most n advances.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "pe_bucket.hpp"

namespace {

int failures = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) { if (++failures <= 20) std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); } \
    } while (0)

const double INF = std::numeric_limits<double>::infinity();

uint64_t bits(double d) {
    uint64_t b;
    std::memcpy(&b, &d, sizeof b);
    return b;
}

// the kernels' bound before pe_bucket.hpp (pe_batch.hip's next_bound and the
// two copies in k_sparse_rows)
double parent_bound(double mn, double delta) {
    double nb = (std::floor(mn / delta) + 1.0) * delta;
    if (!(mn < nb)) nb = mn + delta;
    return nb;
}

long pairs = 0, stalls = 0, step2 = 0;

void check_pair(double mn, double delta) {
    if (!(mn >= 0.0) || !std::isfinite(mn) || !(delta > 0.0)) return;
    ++pairs;
    const double nb = shdpe::bucket_bound(mn, delta);
    const double pb = parent_bound(mn, delta);
    const bool ok = mn < nb;
    CHECK(ok);
    if (!ok && failures <= 20) std::printf("  mn %a delta %a bound %a\n", mn, delta, nb);
    if (mn < pb) {
        CHECK(bits(nb) == bits(pb));
        const double first = (std::floor(mn / delta) + 1.0) * delta;
        if (!(mn < first)) ++step2;
    } else {
        // the last resort: exactly one ulp up
        ++stalls;
        CHECK(bits(nb) == bits(mn) + 1);
        CHECK(nb == std::nextafter(mn, INF));
    }
    if (std::isinf(delta)) CHECK(nb == INF);
}

// The kernels' outer loop over a sorted key list: everything below the bound
// is processed; when nothing is, the bound moves to the minimum key's bucket.
int sweep(const std::vector<double>& keys, double delta) {
    const size_t n = keys.size();
    size_t i = 0;
    int advances = 0;
    double bound = delta;
    while (i < n) {
        while (i < n && keys[i] < bound) ++i;
        if (i == n) break;
        bound = shdpe::bucket_bound(keys[i], delta);
        if (++advances > (int)n) return advances;     // (stalled: the caller's check fails)
    }
    return advances;
}

std::vector<double> mn_values() {
    std::vector<double> v = {0.0, DBL_TRUE_MIN, DBL_MIN, DBL_MAX, std::nextafter(DBL_MAX, 0.0),
                             1.0, 3.0, 1e-3, 0.1, 1000.0, 123456.789, 1e15, 1e16, 1e100, 1e200, 1e-200, 1e300};
    for (int e = -1022; e <= 1023; e += (e > -70 && e < 70) ? 1 : 37) {
        const double p = std::ldexp(1.0, e);
        v.push_back(p);
        v.push_back(std::nextafter(p, INF));
        v.push_back(std::nextafter(p, 0.0));
    }
    return v;
}

std::vector<double> delta_values() {
    std::vector<double> v = {DBL_TRUE_MIN, DBL_MIN, DBL_MAX, 1e-14, 0.75, 16.0, 1.0};
    for (int k = -300; k <= 300; k += 4) {
        const double d = std::pow(10.0, k);
        v.push_back(d);
        v.push_back(std::nextafter(d, INF));
        v.push_back(std::nextafter(d, 0.0));
    }
    for (int e = -1022; e <= 1023; e += 29) v.push_back(std::ldexp(1.0, e));
    return v;
}

}  // namespace

int main() {
    const std::vector<double> mns = mn_values(), deltas = delta_values();

    // adversarial grid
    for (double mn : mns)
        for (double d : deltas) check_pair(mn, d);
    // mn/delta at and beyond 2^53 (where floor(q) + 1 == q), and overflowing
    for (double mn : mns) {
        if (mn == 0.0) continue;
        for (int s : {40, 51, 52, 53, 54, 55, 60, 64, 100, 500, 1000, 1074, 2000}) {
            for (double f : {1.0, 1.5, 0.75, 1.0 / 3.0}) {
                const double d = std::ldexp(mn, -s) * f;
                check_pair(mn, d);
                check_pair(mn, std::nextafter(d, INF));
                check_pair(mn, std::nextafter(d, 0.0));
            }
        }
    }
    CHECK(std::isinf(1e200 / 1e-200));
    check_pair(1e200, 1e-200);
    check_pair(DBL_MAX, DBL_TRUE_MIN);
    // mn = 0: the first bucket is [0, delta)
    for (double d : deltas) CHECK(shdpe::bucket_bound(0.0, d) == d);
    // one bucket
    for (double mn : mns) {
        CHECK(shdpe::bucket_bound(mn, INF) == INF);
        check_pair(mn, INF);
    }

    // random: the widths of a real engine, and the stalling ones
    std::mt19937_64 rng(20240607);
    std::uniform_real_distribution<double> u01(0.0, 1.0);
    long stall14 = 0;
    const long N14 = 200000;
    for (long k = 0; k < N14; ++k) {
        const double mn = 1.0 + 999.0 * u01(rng);
        const long before = stalls;
        check_pair(mn, 1e-14);
        stall14 += stalls - before;
    }
    for (long k = 0; k < 400000; ++k) {
        const double mn = std::pow(10.0, -320.0 + 628.0 * u01(rng));
        const double d = std::pow(10.0, -320.0 + 628.0 * u01(rng));
        check_pair(mn, d);
        // delta near mn's ulp: the border between steps 2 and 3
        const double ulp = std::nextafter(mn, INF) - mn;
        check_pair(mn, ulp * (0.25 + 2.0 * u01(rng)));
        check_pair(mn, ulp * 0.5);
        check_pair(mn, std::nextafter(ulp * 0.5, INF));
    }

    // sweeps over sorted key lists
    int sweeps = 0;
    auto check_sweep = [&](std::vector<double> keys, double d) {
        std::sort(keys.begin(), keys.end());
        const int adv = sweep(keys, d);
        CHECK(adv <= (int)keys.size());
        if (std::isinf(d)) CHECK(adv == 0);
        ++sweeps;
    };
    const std::vector<double> widths = {1e-300, 1e-14, 1e-3, 0.37, 1.0, 16.0, 1e6, 1e300, INF};
    for (int rep = 0; rep < 4; ++rep) {
        std::vector<double> uni(2000), logu(2000), dup(2000), chain(2000);
        for (double& k : uni) k = 1.0 + 999.0 * u01(rng);
        for (double& k : logu) k = std::pow(10.0, -3.0 + 7.0 * u01(rng));
        for (size_t k = 0; k < dup.size(); ++k) dup[k] = (double)(1 + (rng() % 50));     // quantised: ties
        chain[0] = std::ldexp(1.0, 10 * rep) * (1.0 - DBL_EPSILON * 500);               // consecutive doubles across a power of two
        for (size_t k = 1; k < chain.size(); ++k) chain[k] = std::nextafter(chain[k - 1], INF);
        uni[0] = logu[0] = 0.0;                                                           // the source's key
        for (double d : widths) {
            check_sweep(uni, d);
            check_sweep(logu, d);
            check_sweep(dup, d);
            check_sweep(chain, d);
        }
    }

    std::printf("pairs %ld stalls %ld step2 %ld stall14 %ld of %ld sweeps %d\n", pairs, stalls, step2, stall14, N14,
                sweeps);
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
