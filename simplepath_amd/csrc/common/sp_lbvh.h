// sp_lbvh.h -- the arithmetic of the linear BVH build, shared by the host
// restatement (sp_bvh.cpp build_bvh_lbvh) and the device kernels (sp_build.hip) so that both make
// the same tree bit for bit: centroid cells, 63-bit Morton codes, and the Karras (2012) ranges.
#pragma once

#include "sp_box.h"

#include <cstdint>

namespace lbvh {

// Centroid bounds.  The accumulator starts at +-inf and a NaN value never replaces it, so the
// result is the min / max of the ordered values in any reduction order (up to the sign of zero).
SP_HD float lower(float acc, float v) { return (v < acc) ? v : acc; }
SP_HD float upper(float acc, float v) { return (v > acc) ? v : acc; }

// 21-bit cell of a centroid on one axis; a NaN product lands in cell 0 like fmaxf(x, 0) does
SP_HD uint32_t cell(float c, float lo, float hi)
{
    if (!(hi > lo)) return 0u;
    const float x = (c - lo) * (2097152.0f / (hi - lo));
    float       t = (x > 0.0f) ? x : 0.0f;
    t             = (t < 2097151.0f) ? t : 2097151.0f;
    return (uint32_t)t;
}

// bit i of v -> bit 3i
SP_HD uint64_t spread3(uint32_t v)
{
    uint64_t x = v & 0x1fffffu;
    x = (x | x << 32) & 0x001f00000000ffffull;
    x = (x | x << 16) & 0x001f0000ff0000ffull;
    x = (x | x << 8) & 0x100f00f00f00f00full;
    x = (x | x << 4) & 0x10c30c30c30c30c3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}
// x most significant: bit 3i+2 is x, 3i+1 is y, 3i is z
SP_HD uint64_t code(uint32_t qx, uint32_t qy, uint32_t qz) { return spread3(qx) << 2 | spread3(qy) << 1 | spread3(qz); }

// common prefix of the keys (code, position) at sorted positions i and j; equal codes fall back
// to the positions, so all keys are distinct
SP_HD int delta(const uint64_t* codes, int64_t n, int64_t i, int64_t j)
{
    if (j < 0 || j >= n) return -1;
    const uint64_t x = codes[i] ^ codes[j];
    if (x) return __builtin_clzll(x);
    return 64 + __builtin_clz((uint32_t)(i ^ j));
}

// Internal node i of n - 1 (n >= 2): the sorted positions [first, last] it covers and its split
// (left child [first, split], right child [split + 1, last]).  Every loop halves or doubles a
// step below 2n.
struct Range {
    uint32_t first, last, split, axis;
};
SP_HD Range node_range(const uint64_t* codes, int64_t n, int64_t i)
{
    const int64_t d    = (delta(codes, n, i, i + 1) - delta(codes, n, i, i - 1)) >= 0 ? 1 : -1;
    const int     dmin = delta(codes, n, i, i - d);
    int64_t       lmax = 2;
    while (delta(codes, n, i, i + lmax * d) > dmin) lmax *= 2;
    int64_t l = 0;
    for (int64_t t = lmax / 2; t >= 1; t /= 2)
        if (delta(codes, n, i, i + (l + t) * d) > dmin) l += t;
    const int64_t j     = i + l * d;
    const int     dnode = delta(codes, n, i, j);
    int64_t       s = 0, t = l;
    do {
        t = (t + 1) >> 1;
        if (delta(codes, n, i, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    const int64_t g = i + s * d + (d < 0 ? -1 : 0);
    Range         r;
    r.first = (uint32_t)(i < j ? i : j);
    r.last  = (uint32_t)(i < j ? j : i);
    r.split = (uint32_t)g;
    // axis of the highest code bit in which the two sides differ: the left child is its low side
    const uint64_t x = codes[g] ^ codes[g + 1];
    r.axis           = x ? (uint32_t)(2 - (63 - __builtin_clzll(x)) % 3) : 0u;
    return r;
}

// Candidate numbering: internal nodes 0 .. n-2, then the single primitives by sorted position.
SP_HD uint32_t left_cand(const Range& r, uint32_t n) { return r.split == r.first ? (n - 1u) + r.split : r.split; }
SP_HD uint32_t right_cand(const Range& r, uint32_t n) { return r.split + 1u == r.last ? (n - 1u) + r.split + 1u : r.split + 1u; }

} // namespace lbvh
