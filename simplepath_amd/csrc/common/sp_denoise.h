// sp_denoise.h -- the expressions of the edge-avoiding a-trous filter (include/simplepath_hip.h,
// "denoising": THE RULE), shared by the device kernels (sp_denoise.hip) and the host program that
// checks them against the numpy restatement (tests/cpp/denoise_host_main.cpp).  float32, no
// contraction, the operand order of the rule; the only transcendental is lm_expf.
#pragma once

#include "sp_libm.h"

namespace spdn {
using namespace spm;

constexpr float k_albedo_floor = 0.01f; // what a floor of 0 means: conventions, not measurements
constexpr float k_depth_floor  = 1e-3f;
constexpr int   k_max_levels   = 8;

// h[d + 2], d = -2 .. 2: the B3 spline; every product of two entries is exact
SP_HD float spline(int i) { return i == 2 ? 0.375f : ((i == 1 || i == 3) ? 0.25f : 0.0625f); }

// Prepare: the demodulation divisor of one channel (a NaN gives the floor) and the depth gain
SP_HD float albedo_scale(float k, float a, float albedo_floor)
{
    const float s = (k * a) + (1.0f - k);
    return s > albedo_floor ? s : albedo_floor;
}
SP_HD float depth_gain(float z, float sigma_depth, float depth_floor)
{
    return 1.0f / (sigma_depth * (z > depth_floor ? z : depth_floor));
}

// A level's constants, computed once on the host.  A guide that is not given has a factor of +0:
// its term is then (+0 or a finite square) * 0 = +0 on the zeros the prepare kernel stores for it.
struct Level {
    int   step;
    float inv_c, inv_n, inv_k;
};
static inline Level level_constants(int i, float sigma_color, float sigma_normal, float sigma_coverage, bool has_normal,
                                    bool has_coverage)
{
    Level L;
    L.step         = 1 << i;
    const float sc = sigma_color * (1.0f / (float)(1 << i)); // a power of two: exact scaling
    L.inv_c        = 1.0f / (sc * sc);
    L.inv_n        = has_normal ? 1.0f / (sigma_normal * sigma_normal) : 0.0f;
    L.inv_k        = has_coverage ? 1.0f / (sigma_coverage * sigma_coverage) : 0.0f;
    return L;
}

// One pixel as the levels read it: x and z from a colour plane, n and k from the guide record.
struct Pixel {
    float x[3], z, n[3], k;
};

SP_HD float sq3(float d0, float d1, float d2) { return (d0 * d0 + d1 * d1) + d2 * d2; }

// w of the tap q seen from the centre p; g: p's depth gain (+0 without a depth guide)
SP_HD float tap_weight(const Pixel& q, const Pixel& p, float g, const Level& L, float h2)
{
    const float ec = sq3(q.x[0] - p.x[0], q.x[1] - p.x[1], q.x[2] - p.x[2]) * L.inv_c;
    const float en = sq3(q.n[0] - p.n[0], q.n[1] - p.n[1], q.n[2] - p.n[2]) * L.inv_n;
    const float dz = (q.z - p.z) * g;
    const float ed = dz * dz;
    const float dk = q.k - p.k;
    const float ek = (dk * dk) * L.inv_k;
    const float e  = ((ec + en) + ed) + ek;
    return h2 * lm_expf(-e);
}

// The sums of one pixel over a level's counted taps, in tap order
struct Accum {
    float    acc[3] = { 0.0f, 0.0f, 0.0f }, W = 0.0f;
    uint32_t taps   = 0;
};
SP_HD void accumulate(Accum& s, float w, const Pixel& q)
{
    if (!(w > 0.0f)) return; // NaN and 0 fail the comparison
    s.acc[0] = s.acc[0] + w * q.x[0];
    s.acc[1] = s.acc[1] + w * q.x[1];
    s.acc[2] = s.acc[2] + w * q.x[2];
    s.W      = s.W + w;
    ++s.taps;
}
SP_HD float level_result(const Accum& s, int ch, float x_p) { return s.W > 0.0f ? s.acc[ch] / s.W : x_p; }

// the pixel's Morton index in its 8x8 tile: x in the even bits, y in the odd ones
SP_HD uint32_t morton_lane(uint32_t x, uint32_t y)
{
    x &= 7u;
    y &= 7u;
    const uint32_t sx = (x & 1u) | ((x & 2u) << 1) | ((x & 4u) << 2);
    const uint32_t sy = (y & 1u) | ((y & 2u) << 1) | ((y & 4u) << 2);
    return sx | (sy << 1);
}

} // namespace spdn
