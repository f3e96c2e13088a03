// The arithmetic of a moment map that moments.hip and cube_source_maps.hip share (include/kimg.h,
// "Moment maps"): the running sums of one element of the plane, one sample added to them, and the
// sums turned into the maps' values.  Both units compile these expressions, so that a per-source map
// has the bits of kimg_moments on the source's own cube.  Everything here is local to the including
// translation unit.
#pragma once
#include "kimg_cube_column.h"

namespace {

struct mm_acc {
    double S0, S1, S2;
    float peak;
    int n, pc;
};

// One sample: I of channel c with selection value s against the cut ct; d = x[c] - x_ref
template <bool SECOND>
__device__ inline void mm_add(mm_acc &a, float I, double s, double ct, double d, int c)
{
    const bool enter = isfinite(I) && s > ct;
    const double Id = (double) I;
    a.n += enter ? 1 : 0;
    a.S0 = enter ? a.S0 + Id : a.S0;
    if constexpr (SECOND) {
        const double t = Id * d;
        a.S1 = enter ? a.S1 + t : a.S1;
        a.S2 = enter ? a.S2 + t * d : a.S2;
    }
    const bool higher = enter && I > a.peak;
    a.peak = higher ? I : a.peak;
    a.pc = higher ? c : a.pc;
}

// What the sums of one element give, moment 9 excepted (x of channel a.pc, where `any`): the caller
// reads it from its table.
struct mm_values {
    float m0, m1, m2, m8;
    bool any;
};

template <bool SECOND>
__device__ inline mm_values mm_finish(const mm_acc &a, double width, double x_ref)
{
    mm_values v;
    v.any = a.n > 0;
    const bool positive = v.any && a.S0 > 0.0;
    v.m0 = v.any ? (float) (a.S0 * width) : col_nan();
    v.m8 = v.any ? a.peak : col_nan();
    v.m1 = v.m2 = col_nan();
    if constexpr (SECOND) {
        const double r = a.S1 / a.S0;
        const double q = a.S2 / a.S0;
        double var = q - r * r;
        var = var < 0.0 ? 0.0 : var;
        v.m1 = positive ? (float) (x_ref + r) : col_nan();
        v.m2 = positive ? (float) sqrt(var) : col_nan();
    }
    return v;
}

}  // namespace
