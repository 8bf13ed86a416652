// pe_bucket.hpp -- the delta-stepping bucket bound, shared by k_sparse_rows'
// two relax loops and k_batch_rows.  No HIP header: it compiles under hipcc
// (host and device) and under plain g++ (tests/native/bucket_bound.cpp).
#pragma once

#if defined(__HIPCC__)
#define SHDPE_BUCKET_FN __host__ __device__ __forceinline__
#else
#define SHDPE_BUCKET_FN inline
#endif

namespace shdpe {

// The bound of the bucket that holds key mn (finite, >= 0; delta > 0): the
// smallest multiple of delta above it.  Always strictly above mn, so a relax
// loop that raises its bound to this retires at least the minimum key:
//  1. (floor(mn/delta) + 1) * delta -- the multiple, whenever it rounds above mn;
//  2. mn + delta when rounding left step 1 at or below mn (mn/delta past 2^53);
//  3. the next double above mn when delta < ulp(mn)/2 makes step 2 return mn
//     too.  Without it the bound never advances and the loop spins.
// Steps 1 and 2 are the formula the kernels always had: where they succeed
// the result is theirs, bit for bit.
SHDPE_BUCKET_FN double bucket_bound(double mn, double delta) {
    double nb = (__builtin_floor(mn / delta) + 1.0) * delta;
    if (!(mn < nb)) nb = mn + delta;
    if (!(mn < nb)) {
        unsigned long long b;
        __builtin_memcpy(&b, &mn, sizeof b);
        ++b;    // non-negative finite doubles order like their bit patterns
        __builtin_memcpy(&nb, &b, sizeof b);
    }
    return nb;
}

}  // namespace shdpe
