// sp_wide.h -- the per-node arithmetic of the 8-wide collapse, shared by the host
// builders (sp_bvh.cpp build_wide, build_wide_levels) and the device finish (sp_finish.hip) so that
// all three write the same 20 words for the same binary subtree: which children a wide node takes,
// which octant slot each lands in, and the outward power-of-two quantisation of their boxes.
// A node's content depends on its binary root alone; only words 4 and 5 (child_base, leaf_base)
// depend on where the node sits in the whole tree, and the caller sets those.
#pragma once

#include "sp_math.h"

#include <cstdint>

namespace spw {

constexpr uint32_t LEAF       = 0x80000000u;       // sph::BVH_LEAF
constexpr uint32_t CHILD_MASK = (1u << 30) - 1u;   // sph::BVH_CHILD_MASK
constexpr uint32_t MAX_RECORDS = 1u << 24;         // a record index must fit the walk's stack entry
constexpr int      MAX_LEVELS  = 64;

enum Error { OK = 0, ERR_META = 1, ERR_QUANTISE = 2, ERR_RECORDS = 3, ERR_LEVELS = 4, ERR_EMPTY_LEVEL = 5, ERR_LINKS = 6 };
SP_HD const char* error_text(int e)
{
    switch (e) {
    case ERR_META: return "wide BVH: leaf does not fit a meta byte";
    case ERR_QUANTISE: return "wide BVH: cannot quantise child boxes";
    case ERR_RECORDS: return "wide BVH: more than 2^24 nodes";
    case ERR_LEVELS: return "wide BVH: more than 64 levels";
    case ERR_EMPTY_LEVEL: return "wide BVH: a level came back empty before the tree was exhausted";
    case ERR_LINKS: return "wide BVH: the binary links do not form a tree";
    default: return "wide BVH: no error";
    }
}

// one collapsed node: everything but the two bases
struct Collapsed {
    uint32_t w[20];       // the record; w[4] and w[5] are 0
    uint32_t kid[8];      // binary node in slot s (valid where occupied)
    uint32_t imask;       // slots holding an inner child
    uint32_t lmask;       // slots holding a leaf
    int      span;        // child records allocated: last inner slot + 1
    uint32_t own;         // primitives in this node's leaf slots
};

template <typename N>
SP_HD bool is_leaf(const N* nodes, uint32_t i) { return (nodes[i].b & LEAF) != 0; }

template <typename N>
SP_HD float node_area(const N& n)
{
    const float dx = n.hi[0] - n.lo[0], dy = n.hi[1] - n.lo[1], dz = n.hi[2] - n.lo[2];
    if (!(dx >= 0.0f)) return 0.0f;
    return 2.0f * (dx * dy + dy * dz + dz * dx);
}

SP_HD uint32_t f32_bits(float f) { return __builtin_bit_cast(uint32_t, f); }
SP_HD float    bits_f32(uint32_t u) { return __builtin_bit_cast(float, u); }

// The exponent frexpf gives (x = m * 2^e, m in [0.5, 1)); 0 for zero, infinity and NaN like glibc's.
SP_HD int frexp_exp(float x)
{
    const uint32_t u = f32_bits(x) & 0x7fffffffu;
    const int      e = (int)(u >> 23);
    if (u == 0u || e == 255) return 0;
    if (e != 0) return e - 126;
    return (31 - __builtin_clz(u)) - 148; // denormal: u * 2^-149
}
// 2^k for k in [-126, 127]
SP_HD float pow2(int k) { return bits_f32((uint32_t)(k + 127) << 23); }

SP_HD float clamp_byte(float q)
{
    q = (q < 0.0f) ? 0.0f : q;      // std::max(q, 0.0f)
    return (255.0f < q) ? 255.0f : q; // std::min(.., 255.0f)
}

// Quantise one axis of the 8 slots onto origin p with the smallest power-of-two step that keeps
// every decoded box (fma(q, step, p), as the walk decodes it) outside the exact one.  False when no
// step up to 2^127 does.
SP_HD bool quantise(const float* lo, const float* hi, float p, float extent, uint8_t* qlo, uint8_t* qhi, uint8_t& ebyte)
{
    int k = -126;
    if (extent > 0.0f) {
        const int e2 = frexp_exp(extent / 254.0f); // extent/254 < 2^e2
        k            = (e2 < -126) ? -126 : e2;
    }
    for (;; ++k) {
        const float step = pow2(k);
        bool        ok   = true;
        for (int c = 0; c < 8 && ok; ++c) {
            float ql = clamp_byte(__builtin_floorf((lo[c] - p) / step));
            while (ql > 0.0f && spm::fma_f(ql, step, p) > lo[c]) ql -= 1.0f;
            float qh = clamp_byte(__builtin_ceilf((hi[c] - p) / step));
            while (qh < 255.0f && spm::fma_f(qh, step, p) < hi[c]) qh += 1.0f;
            if (spm::fma_f(ql, step, p) > lo[c] || spm::fma_f(qh, step, p) < hi[c]) ok = false;
            qlo[c] = (uint8_t)ql;
            qhi[c] = (uint8_t)qh;
        }
        if (ok) {
            ebyte = (uint8_t)(k + 127);
            return true;
        }
        if (k >= 127) return false;
    }
}

// Collapse the binary subtree at `bi` of a tree of `count` nodes into one wide node.  Returns OK,
// ERR_META, ERR_QUANTISE, or ERR_LINKS for a child index outside the tree.
template <typename N>
SP_HD int collapse(const N* nodes, uint32_t count, uint32_t bi, Collapsed& out)
{
    if (bi >= count) return ERR_LINKS;
    // open the internal child of largest area until 8 children; the right half goes in after the left
    uint32_t kids[8];
    int      n = 0;
    if (is_leaf(nodes, bi)) kids[n++] = bi;
    else {
        kids[n++] = nodes[bi].a & CHILD_MASK;
        kids[n++] = nodes[bi].b;
        if (kids[0] >= count || kids[1] >= count) return ERR_LINKS;
    }
    while (n < 8) {
        int   best = -1;
        float ba   = -1.0f;
        for (int i = 0; i < n; ++i)
            if (!is_leaf(nodes, kids[i]) && node_area(nodes[kids[i]]) > ba) { ba = node_area(nodes[kids[i]]); best = i; }
        if (best < 0) break;
        const uint32_t o = kids[best];
        for (int i = n; i > best + 1; --i) kids[i] = kids[i - 1];
        kids[best]     = nodes[o].a & CHILD_MASK;
        kids[best + 1] = nodes[o].b;
        if (kids[best] >= count || kids[best + 1] >= count) return ERR_LINKS;
        ++n;
    }
    // Slots by octant: slot s takes the child lying towards (+ on axis a iff bit a of s) from
    // the node's centre, so a ray whose direction has sign bits o (bit a: d_a < 0) meets the
    // children roughly near to far in the order slot ^ o = 0, 1, ... (sp_path.hpp key_mask).
    // Greedy assignment of the largest projection first; inner child in slot s is node
    // child_base + s (slots taken by leaves or empty leave holes).
    float ulo[3], uhi[3], cen[8][3];
    for (int a = 0; a < 3; ++a) { ulo[a] = INFINITY; uhi[a] = -INFINITY; }
    for (int c = 0; c < n; ++c)
        for (int a = 0; a < 3; ++a) {
            const float l = nodes[kids[c]].lo[a], h = nodes[kids[c]].hi[a];
            ulo[a]        = (l < ulo[a]) ? l : ulo[a]; // std::min(ulo, l)
            uhi[a]        = (uhi[a] < h) ? h : uhi[a]; // std::max(uhi, h)
            cen[c][a]     = 0.5f * (l + h);
        }
    int  slot_kid[8];
    bool kid_done[8];
    for (int s = 0; s < 8; ++s) { slot_kid[s] = -1; kid_done[s] = false; }
    for (int round = 0; round < n; ++round) {
        int   bc = -1, bs = -1;
        float best = -INFINITY;
        for (int c = 0; c < n; ++c) {
            if (kid_done[c]) continue;
            for (int s = 0; s < 8; ++s) {
                if (slot_kid[s] >= 0) continue;
                float score = 0.0f;
                for (int a = 0; a < 3; ++a) score += ((s >> a) & 1 ? 1.0f : -1.0f) * (cen[c][a] - 0.5f * (ulo[a] + uhi[a]));
                if (bc < 0 || score > best) { best = score; bc = c; bs = s; } // NaN (empty box): any slot
            }
        }
        slot_kid[bs] = bc;
        kid_done[bc] = true;
    }
    uint8_t q[6][8];
    uint8_t eb[3];
    for (int a = 0; a < 3; ++a) {
        float lo[8], hi[8];
        for (int s = 0; s < 8; ++s) {
            const int c = slot_kid[s] >= 0 ? slot_kid[s] : 0; // empty slots: any box (never tested)
            lo[s]       = nodes[kids[c]].lo[a];
            hi[s]       = nodes[kids[c]].hi[a];
        }
        if (!quantise(lo, hi, ulo[a], uhi[a] - ulo[a], q[a], q[3 + a], eb[a])) return ERR_QUANTISE;
    }
    out.imask = 0;
    out.lmask = 0;
    out.span  = 0;
    out.own   = 0;
    for (int s = 0; s < 8; ++s) {
        out.kid[s] = slot_kid[s] >= 0 ? kids[slot_kid[s]] : 0u;
        if (slot_kid[s] < 0) continue;
        if (is_leaf(nodes, out.kid[s])) out.lmask |= 1u << s;
        else { out.imask |= 1u << s; out.span = s + 1; }
    }
    uint8_t meta[8];
    for (int s = 0; s < 8; ++s) {
        meta[s] = 0;
        if (!((out.lmask >> s) & 1u)) continue;
        const uint32_t cnt = nodes[out.kid[s]].b & ~LEAF;
        const uint32_t off = out.own;
        if (cnt == 0 || cnt > 7 || off > 31) return ERR_META;
        meta[s] = (uint8_t)(cnt << 5 | off);
        out.own += cnt;
    }
    uint32_t* w = out.w;
    w[0] = f32_bits(ulo[0]);
    w[1] = f32_bits(ulo[1]);
    w[2] = f32_bits(ulo[2]);
    w[3] = (uint32_t)eb[0] | (uint32_t)eb[1] << 8 | (uint32_t)eb[2] << 16 | out.imask << 24;
    w[4] = 0;
    w[5] = 0;
    w[6] = (uint32_t)meta[0] | (uint32_t)meta[1] << 8 | (uint32_t)meta[2] << 16 | (uint32_t)meta[3] << 24;
    w[7] = (uint32_t)meta[4] | (uint32_t)meta[5] << 8 | (uint32_t)meta[6] << 16 | (uint32_t)meta[7] << 24;
    for (int r = 0; r < 6; ++r)
        for (int h = 0; h < 2; ++h)
            w[8 + 2 * r + h] = (uint32_t)q[r][4 * h] | (uint32_t)q[r][4 * h + 1] << 8 | (uint32_t)q[r][4 * h + 2] << 16 |
                               (uint32_t)q[r][4 * h + 3] << 24;
    return OK;
}

// slot_of entries of a collapsed node placed at leaf_base: wide slot leaf_base + off + j is binary
// slot first + j of the leaf in each leaf slot, in slot order
template <typename N, typename I>
SP_HD void write_slots(const N* nodes, const Collapsed& c, uint32_t leaf_base, I* slot_of)
{
    uint32_t at = leaf_base;
    for (int s = 0; s < 8; ++s) {
        if (!((c.lmask >> s) & 1u)) continue;
        const uint32_t cnt = nodes[c.kid[s]].b & ~LEAF, first = nodes[c.kid[s]].a;
        for (uint32_t j = 0; j < cnt; ++j) slot_of[at++] = (I)(first + j);
    }
}

} // namespace spw
