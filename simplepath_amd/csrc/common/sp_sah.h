// sp_sah.h -- the arithmetic that decides a binned SAH tree, shared by the
// recursive host build (sp_bvh.cpp build_bvh_sah), its level-wise restatement
// (build_bvh_sah_levels) and the device build (sp_sah_build.hip) so that all three make the same
// tree bit for bit: centroids, the bin of a centroid, the two sweeps over 32 bins per axis, the
// leaf / split / median decision and the partition predicate.
#pragma once

#include "sp_box.h"

#include <cmath>
#include <cstdint>

namespace sah {

using spm::Box;
using spm::empty_box;

constexpr int BINS = 32;

// Only finite bounds have an order-independent tree: an infinite or empty bound gives a NaN
// centroid, and folds over NaN are not associative.  The device build refuses such input.
SP_HD bool finite_bounds(const float* lo, const float* hi)
{
    bool ok = true;
    for (int i = 0; i < 3; ++i) ok = ok && std::fabs(lo[i]) < INFINITY && std::fabs(hi[i]) < INFINITY;
    return ok;
}

// bins per unit of centroid extent on an axis with hi > lo
SP_HD float scale(float lo, float hi) { return BINS * (1.0f - 1e-5f) / (hi - lo); }

// Bin of a centroid.  The conversion is spelled out: x86's cvttss2si turns a NaN or a product
// outside int's range into INT_MIN, which the clamp then lifts to bin 0; so does this.
SP_HD int bin_of(float c, float lo, float k)
{
    const float p = (c - lo) * k;
    if (!(p > -1.0f && p < 2147483648.0f)) return 0;
    const int bi = (int)p;
    return bi < 0 ? 0 : (bi > BINS - 1 ? BINS - 1 : bi);
}

SP_HD float area(const Box& b)
{
    const float dx = b.hi[0] - b.lo[0], dy = b.hi[1] - b.lo[1], dz = b.hi[2] - b.lo[2];
    if (!(dx >= 0.0f)) return 0.0f;
    return 2.0f * (dx * dy + dy * dz + dz * dx);
}

struct Best {
    float cost = INFINITY;
    int   dim = -1, bin = -1;
};

// The two sweeps over one axis' bins: the first strict minimum wins, axes in order 0, 1, 2 (the
// caller's loop) and bins in order 0..30.  Counts are converted from the exact integers.
SP_HD void sweep(int d, const int* cnt, const Box* bins, Best& best)
{
    float right_area[BINS];
    int   right_cnt[BINS];
    Box   acc = empty_box();
    int   ac  = 0;
    for (int b = BINS - 1; b > 0; --b) {
        if (cnt[b]) spm::fold(acc, bins[b]);
        ac += cnt[b];
        right_area[b] = area(acc);
        right_cnt[b]  = ac;
    }
    acc = empty_box();
    ac  = 0;
    for (int b = 0; b < BINS - 1; ++b) {
        if (cnt[b]) spm::fold(acc, bins[b]);
        ac += cnt[b];
        if (ac == 0 || right_cnt[b + 1] == 0) continue;
        const float cost = area(acc) * ac + right_area[b + 1] * right_cnt[b + 1];
        if (cost < best.cost) {
            best.cost = cost;
            best.dim  = d;
            best.bin  = b;
        }
    }
}

// What becomes of a node of n > 1 primitives with box bb after the sweeps.  A node visit costs
// one triangle test: a node small enough for a leaf stops when the split does not pay.  MEDIAN:
// all centroids coincide, the range is halved by index and the node carries no axis bits.
enum Decision { LEAF = 0, SPLIT = 1, MEDIAN = 2 };
SP_HD Decision decide(const Box& bb, uint32_t n, uint32_t max_leaf, const Best& best)
{
    const float trav_cost = 1.0f;
    const float leaf_cost = area(bb) * static_cast<float>(n);
    if (best.dim < 0 || (n <= max_leaf && best.cost + trav_cost * area(bb) >= leaf_cost))
        return (best.dim < 0 && n > max_leaf) ? MEDIAN : LEAF;
    return SPLIT;
}

// the partition predicate of a SPLIT: true goes left, and equal keys keep their slot order
SP_HD bool goes_left(float c, float lo, float k, int best_bin) { return bin_of(c, lo, k) <= best_bin; }

} // namespace sah
