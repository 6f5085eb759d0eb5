// sp_nee_black.h -- what direct_nee needs to trace a light sample's shadow ray BEFORE the glossy
// selection-weight estimate, shared by the device (sp_path.hpp direct_nee) and the
// host program that checks it (tests/cpp/nee_black_main.cpp).
//
// Material::eval of a glossy material is finish(P, E, albedo, w): P = mf_pdf(wo, wi), E =
// mf_eval(wo, wi) and the albedo do not depend on the weights w, which come from the 16-sample rho
// estimate.  For a light sample that turns out occluded the value of f is never used; all that is
// left of it is one bit -- is f black? -- that decides whether the shadow ray is counted.  A lane
// with an occluded sample skips the estimate and takes that bit from nee_black_known: black, not
// black, or unknown.  An unknown lane runs the estimate (with a wave vote, SP_NEE_SKIP 1, so does
// its whole wave), so the counters never depend on a lane being lucky.
#pragma once

#include "sp_math.h"

namespace spn {
using namespace spm;

enum : int { NEE_UNKNOWN = 0, NEE_BLACK = 1, NEE_NOT_BLACK = 2 };

constexpr float k_hemi_pdf = 1.0f / (2.0f * k_pi); // k_uniform_hemisphere_pdf

// The faces of the guard.  Inside them the estimate is proven finite, not
// NaN and in [0, k_est_max], and the Lambert term of f a positive normal number.
constexpr float k_wo_y_min   = 0x1p-10f;              // |wo.y| in the shading frame
constexpr float k_wo_len_lo  = 0.998f, k_wo_len_hi = 1.002f; // dot(wo, wo)
constexpr float k_alpha_min  = 0x1p-6f, k_alpha_max = 2.0f;
constexpr float k_ior_min    = 1.0f, k_ior_max = 8.0f;
constexpr float k_r_max      = 16.0f;                 // microfacet colour, per channel
constexpr float k_est_max    = 0x1p32f;               // assumed bound of the estimate's luminance (DESIGN.md §26b proves < 2^15)
constexpr float k_pe_max     = 0x1p30f;               // mf_pdf and each channel of mf_eval
constexpr float k_albedo_max = 0x1p10f, k_albedo_top_min = 0x1p-12f;
constexpr float k_lum_min    = 0x1p-10f, k_lum_max = 0x1p10f; // Lambert luminance A = luminance(albedo * pi)
constexpr float k_coat_min   = 0x1p-30f, k_coat_max = 2.0f;   // |1 - F| when not zero

SP_HD float balance(float p, float inner) { return (inner == 0.0f) ? 0.0f : p / inner; }

// LambertianBRDF::rho_impl's luminance: the second weight's numerator in glossy_weights
SP_HD float lambert_lum(rgb albedo) { return luminance(cscale(albedo, k_pi)); }

// OneSampleMaterial::get_selection_weights from the estimate's luminance r0 and the Lambert one
SP_HD void weights_from(float r0, float A, float w[2])
{
    float sum = 0.0f;
    w[0] = r0;
    sum += w[0];
    w[1] = A;
    sum += w[1];
    w[0] = w[0] / sum;
    w[1] = w[1] / sum;
}

// OneSampleMaterial::eval of the glossy pair from its weight-free parts, then the clearcoat's
// (1 - F) where there is one: the operations of onesample_eval_w and material_eval_local.
SP_HD rgb nee_finish(float P, rgb E, rgb albedo, const float w[2], bool coat, float cf)
{
    const float p0    = P * w[0];
    const float p1    = k_hemi_pdf * w[1];
    const float inner = (0.0f + p0) + p1;
    rgb         r     = mkc(0, 0, 0);
    if (p0 > 0.0f) r = cadd(r, cscale(E, balance(p0, inner)));
    if (p1 > 0.0f) r = cadd(r, cscale(albedo, balance(p1, inner)));
    return coat ? cscale(r, cf) : r;
}

// The part of the guard that makes the estimate finite (§26b): values the lane has before the loop.
SP_HD bool estimate_bounded(f3 wo, float alpha_x, float alpha_y, float ior, rgb R, bool visible_area)
{
    const float l2 = dot(wo, wo);
    bool        ok = visible_area;
    ok = ok && abs_f(wo.y) >= k_wo_y_min && l2 >= k_wo_len_lo && l2 <= k_wo_len_hi;
    ok = ok && alpha_x >= k_alpha_min && alpha_x <= k_alpha_max && alpha_y >= k_alpha_min && alpha_y <= k_alpha_max;
    ok = ok && ior >= k_ior_min && ior <= k_ior_max;
    ok = ok && R.r >= 0.0f && R.r <= k_r_max && R.g >= 0.0f && R.g <= k_r_max && R.b >= 0.0f && R.b <= k_r_max;
    return ok; // a NaN fails its comparison
}

// cblack(nee_finish(P, E, albedo, w, coat, cf)) for EVERY w that weights_from makes of an estimate
// in [0, k_est_max] -- or NEE_UNKNOWN.  bounded: estimate_bounded of this lane.
SP_HD int nee_black_known(bool bounded, float P, rgb E, rgb albedo, float A, bool coat, float cf)
{
    bool ok = bounded;
    ok = ok && P >= 0.0f && P <= k_pe_max;
    ok = ok && E.r >= 0.0f && E.r <= k_pe_max && E.g >= 0.0f && E.g <= k_pe_max && E.b >= 0.0f && E.b <= k_pe_max;
    ok = ok && albedo.r >= 0.0f && albedo.r <= k_albedo_max && albedo.g >= 0.0f && albedo.g <= k_albedo_max &&
         albedo.b >= 0.0f && albedo.b <= k_albedo_max;
    ok = ok && (albedo.r >= k_albedo_top_min || albedo.g >= k_albedo_top_min || albedo.b >= k_albedo_top_min);
    ok = ok && A >= k_lum_min && A <= k_lum_max;
    if (!ok) return NEE_UNKNOWN;
    if (!coat) return NEE_NOT_BLACK;
    if (cf == 0.0f) return NEE_BLACK; // every channel of r is finite: r * 0 is a zero
    const float a = abs_f(cf);
    return (a >= k_coat_min && a <= k_coat_max) ? NEE_NOT_BLACK : NEE_UNKNOWN;
}

} // namespace spn
