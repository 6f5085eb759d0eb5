// sp_wide_visit.h -- the test of one 8-wide node's child boxes against a ray, shared
// by the device walks (sp_path.hpp wide_visit) and the host program that checks it bit for bit
// against the branching form it replaced (tests/cpp/wide_visit_main.cpp).
//
// One exit: all eight slots are decoded and tested, whatever this lane's hold (but for the slots
// that no lane of the wave wants, wave_slots below).  Nothing is branched on per lane --
// a slot that is empty or filtered out is dropped by an integer mask at the end (decoding it is
// harmless: no address depends on it), a failed slab axis only clears `ok` (going on cannot set it
// again), the near / far swap and std::max / std::min are selects, and a slot that does not compete
// for `nearest` has its two ordering comparisons masked, so it changes nothing.  On an incoherent
// walk each lane is at another node, so the branching form's exec-mask regions skipped no work for
// a wave and were paid by every wave.
//
// Every comparison is written as the compare-select it was: the results are the branching form's for
// every bit pattern (NaN and infinite slab distances, tmax = +inf, signed zeros, equal minima); no
// site uses a min / max instruction, whose NaN and signed-zero rules differ from (a < b) ? b : a.
// (visit_plain, at the end of the file, is the form for the rays that cannot make a NaN: it does.)
#pragma once

#include "sp_math.h"

#include <cstdint>

namespace spw {

struct Visit {
    uint32_t inner, leaf; // slot masks of the hit children
    int      nearest;     // inner slot with the smallest entry distance (-1: none)
    float    t_rest;      // smallest entry distance of the other hit inner slots
};

// bit j: byte j of w is not zero
SP_HD uint32_t nonzero_bytes(uint32_t w)
{
    w |= w >> 4;
    w |= w >> 2;
    w |= w >> 1;
    return ((w & 0x01010101u) * 0x00204081u >> 21) & 0xfu; // byte j's bit to position 21 + j: no two terms meet
}

// The slots that some lane of the wave may want: the lanes' common mask when all 64 hold the same
// one (a coherent wave, every lane at one node: camera rays at the root, a scene of a few shapes),
// else all eight.  Wave-uniform, so skipping a slot by it is a scalar branch, not an exec-mask region:
// a wave at one node does not pay for its empty slots, and a wave at 64 nodes pays two instructions.
// Testing a slot nobody wants changes no result (it is masked at the end), so any superset is right;
// the host build returns the mask itself, which puts the skipping under the host test.
SP_HD uint32_t wave_slots(uint32_t valid)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t u = (uint32_t)__builtin_amdgcn_readfirstlane((int)valid);
    return __builtin_amdgcn_ballot_w64(valid != u) == 0ull ? u : 0xffu;
#else
    return valid;
#endif
}

// One axis of the slab test (math/BBox.h:254 operation order): false when the interval is empty.
SP_HD bool visit_axis(float lo, float hi, float o, float inv, float& t0, float& t1)
{
    const float tn = (lo - o) * inv, tf = (hi - o) * inv;
    const bool  swap = tn > tf; // a NaN compares false: no swap
    const float a = swap ? tf : tn, b = swap ? tn : tf;
    t0 = (a < t0) ? t0 : a; // std::max(a, t0)
    t1 = (t1 < b) ? t1 : b; // std::min(b, t1)
    return !(t0 > t1);
}

// w: the node's 20 words (sp_wide.h collapse); o, inv: the ray's origin and 1 / direction.
// NAN_SAFE: see sp_path.hpp wide_visit.
template <bool NAN_SAFE>
SP_HD Visit visit(const uint32_t (&w)[20], float ox, float oy, float oz, float ix, float iy, float iz, float tmin, float tmax,
                  uint32_t filter)
{
    const float    px = spm::u2f(w[0]), py = spm::u2f(w[1]), pz = spm::u2f(w[2]);
    const float    sx = spm::u2f((w[3] & 0xffu) << 23);
    const float    sy = spm::u2f(((w[3] >> 8) & 0xffu) << 23);
    const float    sz = spm::u2f(((w[3] >> 16) & 0xffu) << 23);
    const uint32_t imask = w[3] >> 24;
    const uint32_t valid = (imask | nonzero_bytes(w[6]) | nonzero_bytes(w[7]) << 4) & filter & 0xffu; // occupied and wanted
    const uint32_t ranked = imask & filter; // the slots that compete for `nearest`
    const uint32_t slots = wave_slots(valid);
    uint32_t       hits = 0;
    int            nearest = -1;
    float          best = spm::k_infinite, t_rest = spm::k_infinite;
    auto slot = [&](int k) __attribute__((always_inline)) {
        const int   h = k >> 2, s = 8 * (k & 3);
        const float lx = spm::fma_f((float)((w[8 + h] >> s) & 0xffu), sx, px);
        const float ly = spm::fma_f((float)((w[10 + h] >> s) & 0xffu), sy, py);
        const float lz = spm::fma_f((float)((w[12 + h] >> s) & 0xffu), sz, pz);
        const float hx = spm::fma_f((float)((w[14 + h] >> s) & 0xffu), sx, px);
        const float hy = spm::fma_f((float)((w[16 + h] >> s) & 0xffu), sy, py);
        const float hz = spm::fma_f((float)((w[18 + h] >> s) & 0xffu), sz, pz);
        float       t0 = tmin, t1 = tmax;
        bool        ok = visit_axis(lx, hx, ox, ix, t0, t1);
        ok &= visit_axis(ly, hy, oy, iy, t0, t1);
        ok &= visit_axis(lz, hz, oz, iz, t0, t1);
        if (NAN_SAFE) t0 = (t0 == t0) ? t0 : -spm::k_infinite;
        hits |= ok ? 1u << k : 0u;
        // a slot that does not compete changes nothing: its two comparisons are masked, not its distance
        const bool in = ok & (((ranked >> k) & 1u) != 0u);
        const bool lt = in & (t0 < best); // strict, ascending slots: the lowest slot among equal minima
        const bool lr = in & (t0 < t_rest);
        t_rest  = lt ? best : (lr ? t0 : t_rest); // else std::min(t_rest, t0): a NaN t0 is ignored
        nearest = lt ? k : nearest;
        best    = lt ? t0 : best;
    };
    // Most waves of a walk want all eight slots between them: one block, nothing to branch on.  A wave
    // whose lanes agree on fewer (every lane at one node with empty slots: a scene of a few shapes)
    // steps over the others by scalar branches; one block of eight costs such scenes 2 % of the frame.
    if (slots == 0xffu) {
#pragma unroll
        for (int k = 0; k < 8; ++k) slot(k);
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if ((slots >> k) & 1u) slot(k);
    }
    Visit r;
    r.inner = hits & valid & imask;
    r.leaf  = hits & valid & ~imask;
    if (NAN_SAFE) nearest = ((r.inner != 0u) & (nearest < 0)) ? __builtin_ffs((int)r.inner) - 1 : nearest;
    r.nearest = nearest;
    r.t_rest  = t_rest;
    return r;
}

// ---------------------------------------------------------------- the plain form
// The ray side of visit_plain's contract: a finite origin, a finite non-zero 1 / d on every axis, and
// limits that are no NaN (tmax = +inf is allowed).  One class test per component, on the bits.  The
// walks ask it once per ray, with `inv` as they compute it: d = +-0 and the denormals whose inverse
// overflows are rejected by their infinite inverse, an infinite d by its zero inverse.
SP_HD bool plain_ray(float ox, float oy, float oz, float ix, float iy, float iz, float tmin, float tmax)
{
    const auto finite  = [](float v) { return (spm::f2u(v) & 0x7fffffffu) < 0x7f800000u; };
    const auto nonzero = [](float v) { return ((spm::f2u(v) & 0x7fffffffu) - 1u) < 0x7f7fffffu; }; // finite too
    const auto number  = [](float v) { return (spm::f2u(v) & 0x7fffffffu) <= 0x7f800000u; };
    return finite(ox) && finite(oy) && finite(oz) && nonzero(ix) && nonzero(iy) && nonzero(iz) && number(tmin) && number(tmax);
}

// visit<false> for the rays and nodes that cannot make a NaN, without the work that only a NaN needs.
//
// CONTRACT.  The results are visit<false>'s inner, leaf and nearest exactly, and t_rest equal as a
// float value (==; a zero may carry the other sign), for every input with all of:
//   * o.x/y/z finite            -- an infinite origin makes inf - inf against a box that decodes to inf;
//   * inv.x/y/z finite, non-zero -- the only NaN of a slab is 0 * inf (origin in a box plane, 1 / d
//                                  infinite); a zero inverse makes the same NaN from an overflowed box;
//                                  with neither, (lo - o) * inv and (hi - o) * inv are ordered by the
//                                  sign of inv alone, which is what lets near / far be chosen first;
//   * tmin, tmax not NaN        -- min / max instructions drop a NaN operand, (a < b) ? b : a keeps one;
//   * the node's origin finite  -- else lo and hi are NaN or inf - inf;
//   * scale bytes <= 254        -- byte 255 decodes to an infinite step: 0 * inf for a zero byte;
//   * qlo <= qhi on every axis of every occupied-and-wanted slot -- then lo <= hi (fma(q, step, p) is
//     monotone in q), so no swap by value is ever needed.  Every builder keeps this (quantise floors
//     qlo and ceils qhi; tests/test_wide_node_invariant.py), and slots outside `valid` are masked.
// Nothing is claimed outside it: the walks take this form only when spw::plain_ray holds for every
// lane of the wave (sp_path.hpp), and the ray-query kernels never do.
//
// What changes against visit (everything else is visit's, line for line):
//   1. near / far are chosen by the sign of inv on the packed words: 12 selects per visit, not a
//      compare and two selects per axis per slot;
//   2. t0 = max(max3(near x, y, z), tmin), t1 = min(min3(far x, y, z), tmax): with no NaN operand the
//      compare-select chains' value, but for a zero's sign -- which nothing downstream reads (t0 only
//      meets <, and t_rest only > in the closest-hit walk);
//   3. one !(t0 > t1) per slot: t0 only rises and t1 only falls along the axes, so the last interval
//      test implies the first two.
// The block of eight only: a wave that agrees on fewer slots keeps visit's skipping form.
SP_HD float max_plain(float a, float b) { return __builtin_fmaxf(a, b); }
SP_HD float min_plain(float a, float b) { return __builtin_fminf(a, b); }

// One visit of a walk whose wave has voted: `plain` must be wave-uniform on the device.  True: visit_plain
// (below); false: visit<false>, word for word.  One function, so that the two blocks of eight share
// the decode, the skipping form and the exit, and the vote is a scalar branch around straight-line code.
SP_HD Visit visit_voted(bool plain, const uint32_t (&w)[20], float ox, float oy, float oz, float ix, float iy, float iz, float tmin,
                        float tmax, uint32_t filter)
{
    const float    px = spm::u2f(w[0]), py = spm::u2f(w[1]), pz = spm::u2f(w[2]);
    const float    sx = spm::u2f((w[3] & 0xffu) << 23);
    const float    sy = spm::u2f(((w[3] >> 8) & 0xffu) << 23);
    const float    sz = spm::u2f(((w[3] >> 16) & 0xffu) << 23);
    const uint32_t imask = w[3] >> 24;
    const uint32_t valid = (imask | nonzero_bytes(w[6]) | nonzero_bytes(w[7]) << 4) & filter & 0xffu; // occupied and wanted
    const uint32_t ranked = imask & filter; // the slots that compete for `nearest`
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t slots = wave_slots(valid);
#else
    const uint32_t slots = plain ? 0xffu : wave_slots(valid); // the host test runs the plain block on every pair, as an incoherent wave does
#endif
    uint32_t       hits = 0;
    int            nearest = -1;
    float          best = spm::k_infinite, t_rest = spm::k_infinite;
    auto rank = [&](int k, bool ok, float t0) __attribute__((always_inline)) { // visit's update, word for word
        hits |= ok ? 1u << k : 0u;
        const bool in = ok & (((ranked >> k) & 1u) != 0u);
        const bool lt = in & (t0 < best); // strict, ascending slots: the lowest slot among equal minima
        const bool lr = in & (t0 < t_rest);
        t_rest  = lt ? best : (lr ? t0 : t_rest);
        nearest = lt ? k : nearest;
        best    = lt ? t0 : best;
    };
    auto slot = [&](int k) __attribute__((always_inline)) { // visit's slot
        const int   h = k >> 2, s = 8 * (k & 3);
        const float lx = spm::fma_f((float)((w[8 + h] >> s) & 0xffu), sx, px);
        const float ly = spm::fma_f((float)((w[10 + h] >> s) & 0xffu), sy, py);
        const float lz = spm::fma_f((float)((w[12 + h] >> s) & 0xffu), sz, pz);
        const float hx = spm::fma_f((float)((w[14 + h] >> s) & 0xffu), sx, px);
        const float hy = spm::fma_f((float)((w[16 + h] >> s) & 0xffu), sy, py);
        const float hz = spm::fma_f((float)((w[18 + h] >> s) & 0xffu), sz, pz);
        float       t0 = tmin, t1 = tmax;
        bool        ok = visit_axis(lx, hx, ox, ix, t0, t1);
        ok &= visit_axis(ly, hy, oy, iy, t0, t1);
        ok &= visit_axis(lz, hz, oz, iz, t0, t1);
        rank(k, ok, t0);
    };
    if (slots != 0xffu) { // visit's skipping form, whatever the vote
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if ((slots >> k) & 1u) slot(k);
    } else if (!plain) {
#pragma unroll
        for (int k = 0; k < 8; ++k) slot(k);
    } else {
        // the rows the ray enters and leaves by: lower and upper bytes exchanged where it runs backwards
        const bool     bx = ix < 0.0f, by = iy < 0.0f, bz = iz < 0.0f;
        const uint32_t nx[2] = { bx ? w[14] : w[8], bx ? w[15] : w[9] }, fx[2] = { bx ? w[8] : w[14], bx ? w[9] : w[15] };
        const uint32_t ny[2] = { by ? w[16] : w[10], by ? w[17] : w[11] }, fy[2] = { by ? w[10] : w[16], by ? w[11] : w[17] };
        const uint32_t nz[2] = { bz ? w[18] : w[12], bz ? w[19] : w[13] }, fz[2] = { bz ? w[12] : w[18], bz ? w[13] : w[19] };
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int   h = k >> 2, s = 8 * (k & 3);
            const float ax = (spm::fma_f((float)((nx[h] >> s) & 0xffu), sx, px) - ox) * ix;
            const float ay = (spm::fma_f((float)((ny[h] >> s) & 0xffu), sy, py) - oy) * iy;
            const float az = (spm::fma_f((float)((nz[h] >> s) & 0xffu), sz, pz) - oz) * iz;
            const float cx = (spm::fma_f((float)((fx[h] >> s) & 0xffu), sx, px) - ox) * ix;
            const float cy = (spm::fma_f((float)((fy[h] >> s) & 0xffu), sy, py) - oy) * iy;
            const float cz = (spm::fma_f((float)((fz[h] >> s) & 0xffu), sz, pz) - oz) * iz;
            const float t0 = max_plain(max_plain(max_plain(ax, ay), az), tmin);
            const float t1 = min_plain(min_plain(min_plain(cx, cy), cz), tmax);
            rank(k, !(t0 > t1), t0);
        }
    }
    Visit r;
    r.inner   = hits & valid & imask;
    r.leaf    = hits & valid & ~imask;
    r.nearest = nearest;
    r.t_rest  = t_rest;
    return r;
}

SP_HD Visit visit_plain(const uint32_t (&w)[20], float ox, float oy, float oz, float ix, float iy, float iz, float tmin, float tmax,
                        uint32_t filter)
{
    return visit_voted(true, w, ox, oy, oz, ix, iy, iz, tmin, tmax, filter);
}

} // namespace spw
