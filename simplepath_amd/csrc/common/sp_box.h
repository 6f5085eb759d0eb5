// sp_box.h -- the box arithmetic every BVH stage shares, host and device (sp_lbvh.h, sp_sah.h,
// sp_refit.h and their users): an axis-aligned box, its fold into an accumulator, a centroid
// coordinate, and the layout of a primitive's code.
#pragma once

#include "sp_math.h"

#include <cmath>
#include <cstdint>

namespace spm {

// a primitive's code is kind << 30 | index (sp_device.hpp spd::CODE_SHIFT; sp_capi.hip code_of)
constexpr uint32_t CODE_SHIFT    = 30;
constexpr uint32_t CODE_MASK     = (1u << CODE_SHIFT) - 1u;
constexpr uint32_t KIND_TRIANGLE = 0u; // SP_PRIM_TRIANGLE

struct Box { // sph::PrimBounds
    float lo[3], hi[3];
};

SP_HD Box empty_box()
{
    Box b;
    for (int i = 0; i < 3; ++i) {
        b.lo[i] = INFINITY;
        b.hi[i] = -INFINITY;
    }
    return b;
}

// merge (math/BBox.h:192) with _mm_min_ps / _mm_max_ps operand order: the accumulator comes first,
// so on an exact tie between +0 and -0 the later operand wins
SP_HD void fold(Box& acc, const float* lo, const float* hi)
{
    for (int i = 0; i < 3; ++i) {
        acc.lo[i] = sse_min(acc.lo[i], lo[i]);
        acc.hi[i] = sse_max(acc.hi[i], hi[i]);
    }
}
SP_HD void fold(Box& acc, const Box& b) { fold(acc, b.lo, b.hi); }

SP_HD float centre(float lo, float hi) { return (lo + hi) / 2.0f; } // sp_bvh.cpp center_of

} // namespace spm
