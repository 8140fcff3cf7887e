// What the percentile selects share (pch_filter.hip on float32 values, pch_frame.hip on LAS integers): numpy's index
// arithmetic for the 'linear' rule on float32 data, and its interpolation.
#pragma once
#include "pch_common.h"
#include <math.h>

namespace pch {

// host side of np.percentile's index arithmetic (float32 under NEP 50)
struct PctIndex { int64_t k0; int same; float gamma; };
static inline PctIndex pct_index(int64_t n, double q_percent) {
    PctIndex r;
    const float q = (float)q_percent / 100.0f;          // np.true_divide(q, float32(100))
    const float vi = (float)(n - 1) * q;                // (n - 1) * quantiles -> float32
    float prev = floorf(vi);
    r.gamma = vi - prev;
    r.same = 0;
    if (vi >= (float)(n - 1)) { prev = (float)(n - 1); r.same = 1; }   // indexes -> -1 (last)
    if (vi < 0.0f) { prev = 0.0f; r.same = 1; }
    int64_t k0 = (int64_t)prev;
    if (k0 > n - 1) k0 = n - 1;                          // float32(n-1) may round up
    if (k0 < 0) k0 = 0;
    if (k0 == n - 1) r.same = 1;
    r.k0 = k0;
    return r;
}

#ifdef __HIPCC__
// numpy's _lerp in float32: a + (b-a)*t, and b - (b-a)*(1-t) where t >= 0.5
// (numpy/lib/_function_base_impl.py:4639-4660)
__device__ __forceinline__ float sel_lerp_f32(float a, float b, float gamma) {
    const float diff = b - a;
    float r = a + diff * gamma;
    if (gamma >= 0.5f) r = b - diff * (1.0f - gamma);
    return r;
}
#endif

}  // namespace pch
