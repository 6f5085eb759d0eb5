// sp_refit.h -- the per-element arithmetic of a BVH refit, shared by the host
// restatement (sp_bvh.cpp refit_wide, sp_capi.hip refit_host) and the device kernels (sp_refit.hip)
// so that both write the same bytes for the same topology and the same new positions: a primitive's
// bounds, the fold of a leaf, the merge of two children, and the words of an 8-wide record from the
// exact boxes of its slots.  Nothing here looks at the boxes a tree held before.
#pragma once

#include "sp_box.h"
#include "sp_wide.h"

namespace spr {

using spm::Box;
using spm::empty_box;
using spm::fold; // a leaf's fold (lb_emit, sph::lbvh_fit_boxes): the box so far is the first operand

// BBox::extend by a point (shapes/Triangle.h:228): min(p, m_min), max(p, m_max)
SP_HD void extend(Box& b, float x, float y, float z)
{
    const float v[3] = { x, y, z };
    for (int i = 0; i < 3; ++i) {
        b.lo[i] = spm::sse_min(v[i], b.lo[i]);
        b.hi[i] = spm::sse_max(v[i], b.hi[i]);
    }
}

// a triangle's bounds from its three positions (3 floats each), vertex 0 first
SP_HD Box tri_box(const float* p0, const float* p1, const float* p2)
{
    Box b = empty_box();
    extend(b, p0[0], p0[1], p0[2]);
    extend(b, p1[0], p1[1], p1[2]);
    extend(b, p2[0], p2[1], p2[2]);
    return b;
}

// ---- 8-wide records (sp_host.hpp WideBvh: 20 words) ------------------------------------------------
SP_HD uint32_t rec_imask(const uint32_t* w) { return w[3] >> 24; }
SP_HD uint32_t rec_meta(const uint32_t* w, int s) { return (w[6 + s / 4] >> (8 * (s % 4))) & 0xffu; }
// slots that hold something: an inner child or a leaf
SP_HD uint32_t rec_occupied(const uint32_t* w)
{
    uint32_t m = rec_imask(w);
    for (int s = 0; s < 8; ++s)
        if (rec_meta(w, s) != 0u) m |= 1u << s;
    return m;
}

// The record's words from the exact boxes of its occupied slots: the union (the comparisons of
// spw::collapse, ascending slot order) goes to `u` and, as the grid origin, to w[0..2]; each axis is
// quantised onto it (an empty slot is given the box of the lowest occupied one: never tested); the
// three exponent bytes of w[3] and w[8..19] are rewritten, the imask byte and w[4..7] stay.  A record
// without an occupied slot (a hole) is left alone, its union empty.  spw::OK or spw::ERR_QUANTISE.
SP_HD int refit_record(uint32_t* w, const Box* slot, uint32_t occupied, Box& u)
{
    u = empty_box();
    if ((occupied & 0xffu) == 0u) return spw::OK;
    int first = 0;
    while (!((occupied >> first) & 1u)) ++first;
    for (int s = 0; s < 8; ++s) {
        if (!((occupied >> s) & 1u)) continue;
        for (int a = 0; a < 3; ++a) {
            const float l = slot[s].lo[a], h = slot[s].hi[a];
            u.lo[a]       = (l < u.lo[a]) ? l : u.lo[a];
            u.hi[a]       = (u.hi[a] < h) ? h : u.hi[a];
        }
    }
    uint8_t q[6][8];
    uint8_t eb[3];
    for (int a = 0; a < 3; ++a) {
        float lo[8], hi[8];
        for (int s = 0; s < 8; ++s) {
            const int c = ((occupied >> s) & 1u) ? s : first;
            lo[s]       = slot[c].lo[a];
            hi[s]       = slot[c].hi[a];
        }
        if (!spw::quantise(lo, hi, u.lo[a], u.hi[a] - u.lo[a], q[a], q[3 + a], eb[a])) return spw::ERR_QUANTISE;
    }
    w[0] = spw::f32_bits(u.lo[0]);
    w[1] = spw::f32_bits(u.lo[1]);
    w[2] = spw::f32_bits(u.lo[2]);
    w[3] = (uint32_t)eb[0] | (uint32_t)eb[1] << 8 | (uint32_t)eb[2] << 16 | (w[3] & 0xff000000u);
    for (int r = 0; r < 6; ++r)
        for (int h = 0; h < 2; ++h)
            w[8 + 2 * r + h] = (uint32_t)q[r][4 * h] | (uint32_t)q[r][4 * h + 1] << 8 | (uint32_t)q[r][4 * h + 2] << 16 |
                               (uint32_t)q[r][4 * h + 3] << 24;
    return spw::OK;
}

} // namespace spr
