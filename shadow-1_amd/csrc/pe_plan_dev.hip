// pe_plan_dev.hip -- the batch plan of batch order 2 composed on the device:
// what batch_order_cost (pe_plan.cpp) does on one host thread, from the
// positions already uploaded for the relax, on the shard's stream ahead of it,
// so that no host planning and no upload stands between a compute call and
// its first kernel.  Four steps, ordered by the stream alone:
//   compose   the positions stably sorted by rank (radix sort on the rank: the
//             sort is stable, so equal ranks keep their sequence in pos[]);
//   batch     one wave per batch of LB consecutive rows: the lanes' bucket key
//             offsets (lane_offsets) and the predicted cost, every sum in the
//             host's sequence -- built with -ffp-contract=off, so each
//             operation rounds as the host's does;
//   sequence  the batches stably sorted by descending cost (radix sort on the
//             cost's bits: every cost is positive);
//   emit      rows and offsets permuted into the arrays k_batch_rows reads, and
//             the control words of the call that the host used to clear.
// The host path stays (orders 0 and 1, shd_pe_get_paths, SHDPE_DEVICE_PLAN=0)
// and is the reference of tests/test_gpu_device_plan.py.
#include <hip/hip_runtime.h>

#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>

#include "pe_engine.hpp"

namespace shdpe {

static constexpr int PLAN_THREADS = 256;
static constexpr int WAVE = 64;

__global__ void k_plan_keys(const int32_t* __restrict__ rank, const int32_t* __restrict__ pos, int32_t cnt,
                            uint32_t* __restrict__ key) {
    const int32_t i = blockIdx.x * PLAN_THREADS + threadIdx.x;
    if (i < cnt) key[i] = (uint32_t)rank[pos[i]];
}

// (v > 0 ? v : 0: std::max(0.0, v) of the host)
__device__ static inline double at_least_zero(double v) { return 0.0 < v ? v : 0.0; }

// One wave per batch b: lane t < LB holds the batch's row t (-1 pads, as the
// sorted rows run out), lane j < G the sums of hub group j.  Every loop below
// is uniform over the wave (the shuffles need all lanes).
__global__ void k_plan_batch(DevPlan dp, int32_t cnt, int32_t nB, int32_t LB, int32_t kind, double c0, double cOff,
                             double cSpread) {
    const int32_t b = blockIdx.x * (PLAN_THREADS / WAVE) + threadIdx.x / WAVE;
    if (b >= nB) return;
    const int t = threadIdx.x % WAVE;
    const int G = dp.G;
    const int64_t at = (int64_t)b * LB + t;
    const int32_t p = t < LB && at < cnt ? dp.sorted[at] : -1;
    const bool real = p >= 0;
    const double ro = real ? dp.rowOff[p] : 0.0;
    const double* dist = dp.hubDist + (real ? (int64_t)p * G : 0);
    // offsets: S = the lane's sum over the groups that reach every real lane
    double S = 0.0;
    int nJ = 0;
    for (int j = 0; kind == 1 && j < G; ++j) {
        const double d = real ? dist[j] : 0.0;
        if (!__all(!real || isfinite(d))) continue;
        ++nJ;
        if (real) S += d;
    }
    double off = ro;               // no common group (or kind 0): the nearest-hub distance
    if (nJ) {
        double mn = real ? S : INFINITY;
        for (int w = WAVE / 2; w > 0; w >>= 1) mn = fmin(mn, __shfl_xor(mn, w));
        off = (S - mn) / nJ;
    }
    if (t < LB) {
        dp.rowsTmp[at] = p;
        dp.offTmp[at] = real ? off : 0.0;
    }
    // cost: per group the sum and the sum of squares of (distance - rowOff) /
    // unit over the lanes ascending; the lanes' rowOff summed ascending
    double sum = 0.0, sumSq = 0.0, offSum = 0.0;
    int cntOf = 0, lanes = 0;
    for (int l = 0; l < LB; ++l) {
        const int32_t pl = __shfl(p, l);
        const double rl = __shfl(ro, l);
        if (pl < 0) continue;      // (uniform: pl is the same in every lane)
        ++lanes;
        offSum += rl;
        const double d = t < G ? dp.hubDist[(int64_t)pl * G + t] : INFINITY;
        if (isfinite(d)) {
            const double x = (d - rl) / dp.unit;
            sum += x;
            sumSq += x * x;
            ++cntOf;
        }
    }
    double var = 0.0;
    int terms = 0;
    for (int j = 0; j < G; ++j) {
        const double sj = __shfl(sum, j), qj = __shfl(sumSq, j);
        const int cj = __shfl(cntOf, j);
        if (!cj) continue;
        var += at_least_zero(qj - sj * sj / cj);
        terms += cj;
    }
    if (t) return;
    const double spread = terms ? sqrt(var / terms) : 0.0;
    const double meanOff = lanes ? offSum / lanes / dp.unit : 0.0;
    dp.cost[b] = (c0 + cOff * meanOff + cSpread * spread) * lanes / LB;
    dp.idx[b] = b;
}

// Batch i of the call = composed batch perm[i]; then the call's control words.
__global__ void k_plan_emit(DevPlan dp, int32_t nB, int32_t LB, int32_t* __restrict__ batchRows,
                            double* __restrict__ laneOff, PlanControl ctl) {
    const int64_t stride = (int64_t)gridDim.x * PLAN_THREADS;
    const int64_t t0 = (int64_t)blockIdx.x * PLAN_THREADS + threadIdx.x;
    for (int64_t i = t0; i < (int64_t)nB * LB; i += stride) {
        const int64_t from = (int64_t)dp.perm[i / LB] * LB + i % LB;
        batchRows[i] = dp.rowsTmp[from];
        laneOff[i] = dp.offTmp[from];
    }
    for (int64_t i = t0; i < ctl.tieReqWords; i += stride) ctl.tieReq[i] = -1;
    for (int64_t i = t0; i < ctl.dbgWords; i += stride) ctl.dbg[i] = 0;
    if (t0) return;
    *ctl.next = 0;                 // (for the unsplit kernel's one launch; batch_rounds clears it per launch itself)
    if (ctl.redo) ctl.redo[0] = ctl.redo[1] = 0;
    if (ctl.predCnt) ctl.predCnt[0] = ctl.predCnt[1] = 0;
    if (ctl.tieCount) *ctl.tieCount = 0;
}

static unsigned bits_of(uint32_t maxValue) {
    unsigned b = 1;
    while (b < 32 && (maxValue >> b)) ++b;
    return b;
}

size_t plan_dev_temp_bytes(int32_t maxRows, int32_t maxBatches) {
    size_t a = 0, b = 0;
    if (rocprim::radix_sort_pairs(nullptr, a, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const int32_t*)nullptr,
                                  (int32_t*)nullptr, (size_t)maxRows, 0, 32, nullptr) != hipSuccess ||
        rocprim::radix_sort_pairs_desc(nullptr, b, (const double*)nullptr, (double*)nullptr, (const int32_t*)nullptr,
                                       (int32_t*)nullptr, (size_t)maxBatches, 0, 64, nullptr) != hipSuccess)
        return 0;
    return std::max<size_t>(std::max(a, b), 16);
}

int launch_plan_dev(const DevPlan& dp, const int32_t* dPos, int32_t cnt, int32_t LB, int32_t kind,
                    int32_t* dBatchRows, double* dLaneOff, const PlanControl& ctl, hipStream_t st) {
    if (cnt < 1 || LB < 1 || LB > WAVE || dp.G < 1 || dp.G > WAVE || cnt > dp.capRows) return SHD_PE_EINVAL;
    const int32_t nB = (cnt + LB - 1) / LB;
    // (rowsTmp / offTmp and the caller's arrays hold capRows + 64 entries)
    if (nB > dp.capBatches || (int64_t)nB * LB > (int64_t)dp.capRows + 64) return SHD_PE_EINVAL;
    hipLaunchKernelGGL(k_plan_keys, dim3((cnt + PLAN_THREADS - 1) / PLAN_THREADS), dim3(PLAN_THREADS), 0, st,
                       dp.rank, dPos, cnt, dp.keyIn);
    // The storage was sized for the largest call.  rocPRIM picks its algorithm
    // by the size, and nothing in its interface promises that a smaller sort
    // never asks for more, so each sort is preceded by its size query (host
    // arithmetic, no launch) and a call that would not fit is refused.
    size_t need = 0, have = dp.tempBytes;
    const unsigned rankBits = bits_of((uint32_t)std::max(dp.T - 1, 1));
    if (rocprim::radix_sort_pairs(nullptr, need, dp.keyIn, dp.keyOut, dPos, dp.sorted, (size_t)cnt, 0, rankBits,
                                  st) != hipSuccess || need > have)
        return SHD_PE_ENOMEM;
    if (rocprim::radix_sort_pairs(dp.temp, have, dp.keyIn, dp.keyOut, dPos, dp.sorted, (size_t)cnt, 0, rankBits,
                                  st) != hipSuccess)
        return SHD_PE_EHIP;
    const int perBlock = PLAN_THREADS / WAVE;
    hipLaunchKernelGGL(k_plan_batch, dim3((nB + perBlock - 1) / perBlock), dim3(PLAN_THREADS), 0, st, dp, cnt, nB,
                       LB, kind, COST_C0, COST_OFF, COST_SPREAD);
    have = dp.tempBytes;
    if (rocprim::radix_sort_pairs_desc(nullptr, need, dp.cost, dp.costSorted, dp.idx, dp.perm, (size_t)nB, 0, 64,
                                       st) != hipSuccess || need > have)
        return SHD_PE_ENOMEM;
    if (rocprim::radix_sort_pairs_desc(dp.temp, have, dp.cost, dp.costSorted, dp.idx, dp.perm, (size_t)nB, 0, 64,
                                       st) != hipSuccess)
        return SHD_PE_EHIP;
    const int64_t work = std::max<int64_t>((int64_t)nB * LB, std::max(ctl.tieReqWords, ctl.dbgWords));
    const int grid = (int)std::min<int64_t>(1024, (work + PLAN_THREADS - 1) / PLAN_THREADS);
    hipLaunchKernelGGL(k_plan_emit, dim3(grid), dim3(PLAN_THREADS), 0, st, dp, nB, LB, dBatchRows, dLaneOff, ctl);
    return hipGetLastError() == hipSuccess ? SHD_PE_OK : SHD_PE_EHIP;
}

}  // namespace shdpe
