// sp_bvh.cpp -- bounding volume hierarchies over the bounded primitives.
//
// build_bvh_reference restates shapes/BVHAccelerator.h:173 `construct` exactly (same split
// axis, same split position, libstdc++ std::partition element order, same leaf contents and
// order) so a depth-first, child-0-first traversal visits primitives in the reference's order
// and resolves equal-distance ties identically.  build_bvh_sah is the throughput build: binned
// SAH (Wald 2007) with the same node format; it changes only the visiting order.
#include "sp_host.hpp"
#include "../common/sp_lbvh.h"
#include "../common/sp_sah.h"
#include "../common/sp_wide.h"
#include "../common/sp_refit.h"

#include <cstdio>
#include <cstdlib>

#include <stdexcept>
#include <cstring>

#include <algorithm>
#include <cmath>
#include <functional>

namespace sph {

namespace {
using spm::Box;
using spm::empty_box;
static_assert(spw::LEAF == BVH_LEAF && spw::CHILD_MASK == BVH_CHILD_MASK, "sp_wide.h reads sph::BvhNode links");
// merge (math/BBox.h:192) with _mm_min_ps / _mm_max_ps operand order
Box merge(const Box& a, const PrimBounds& b)
{
    Box r;
    for (int i = 0; i < 3; ++i) {
        r.lo[i] = spm::sse_min(a.lo[i], b.lo[i]);
        r.hi[i] = spm::sse_max(a.hi[i], b.hi[i]);
    }
    return r;
}
float center_of(const PrimBounds& b, int d) { return (b.lo[d] + b.hi[d]) / 2.0f; }

struct RefBuilder {
    const std::vector<PrimBounds>& bounds;
    std::vector<int32_t>           ids;
    std::vector<BvhNode>           nodes;
    int                            max_depth = 0;

    uint32_t build(size_t first, size_t last, int depth)
    {
        max_depth = std::max(max_depth, depth);
        Box bb    = empty_box();
        for (size_t i = first; i < last; ++i) bb = merge(bb, bounds[ids[i]]);
        const uint32_t me = static_cast<uint32_t>(nodes.size());
        nodes.push_back(BvhNode{});
        auto make_leaf = [&]() {
            BvhNode& n = nodes[me];
            for (int i = 0; i < 3; ++i) { n.lo[i] = bb.lo[i]; n.hi[i] = bb.hi[i]; }
            n.a = static_cast<uint32_t>(first);
            n.b = static_cast<uint32_t>(last - first) | BVH_LEAF;
            return me;
        };
        if (last - first <= 4) return make_leaf();
        // max_dim(bounds.size()) (math/Vector3.h:654)
        const float sx = std::fabs(bb.hi[0] - bb.lo[0]);
        const float sy = std::fabs(bb.hi[1] - bb.lo[1]);
        const float sz = std::fabs(bb.hi[2] - bb.lo[2]);
        int         dim;
        if (sx > sy) dim = (sx > sz) ? 0 : 2;
        else dim = (sy > sz) ? 1 : 2;
        const float split_point = (bb.lo[dim] + bb.hi[dim]) / 2.0f;
        const size_t split = stl_partition(ids, first, last, [&](int32_t id) { return center_of(bounds[id], dim) < split_point; });
        if (split == first || split == last) return make_leaf();
        const uint32_t l = build(first, split, depth + 1);
        const uint32_t r = build(split, last, depth + 1);
        BvhNode& n = nodes[me];
        for (int i = 0; i < 3; ++i) { n.lo[i] = bb.lo[i]; n.hi[i] = bb.hi[i]; }
        n.a = l;
        n.b = r;
        return me;
    }
};
} // namespace

Bvh build_bvh_reference(const std::vector<PrimBounds>& bounds)
{
    Bvh        out;
    RefBuilder b{ bounds, {}, {} };
    b.ids.resize(bounds.size());
    for (size_t i = 0; i < bounds.size(); ++i) b.ids[i] = static_cast<int32_t>(i);
    if (!bounds.empty()) b.build(0, bounds.size(), 1);
    out.nodes      = std::move(b.nodes);
    out.prim_order = std::move(b.ids);
    out.max_depth  = b.max_depth;
    return out;
}

// ------------------------------------------------------------------------------ binned SAH
namespace {
struct SahBuilder {
    const std::vector<PrimBounds>& bounds;
    std::vector<int32_t>           ids;
    std::vector<float>             cx, cy, cz;
    std::vector<BvhNode>           nodes;
    int                            max_leaf;
    int                            max_depth = 0;

    const float* cen(int d) const { return d == 0 ? cx.data() : (d == 1 ? cy.data() : cz.data()); }

    uint32_t build(size_t first, size_t last, int depth)
    {
        max_depth = std::max(max_depth, depth);
        Box bb = empty_box(), cb = empty_box();
        for (size_t i = first; i < last; ++i) {
            const int32_t id = ids[i];
            bb               = merge(bb, bounds[id]);
            PrimBounds c;
            c.lo[0] = c.hi[0] = cx[id];
            c.lo[1] = c.hi[1] = cy[id];
            c.lo[2] = c.hi[2] = cz[id];
            cb = merge(cb, c);
        }
        const uint32_t me = static_cast<uint32_t>(nodes.size());
        nodes.push_back(BvhNode{});
        const size_t n = last - first;
        auto make_leaf = [&]() {
            BvhNode& nd = nodes[me];
            for (int i = 0; i < 3; ++i) { nd.lo[i] = bb.lo[i]; nd.hi[i] = bb.hi[i]; }
            nd.a = static_cast<uint32_t>(first);
            nd.b = static_cast<uint32_t>(n) | BVH_LEAF;
            return me;
        };
        if (n <= 1) return make_leaf();
        sah::Best best;
        for (int d = 0; d < 3; ++d) {
            const float lo = cb.lo[d], hi = cb.hi[d];
            if (!(hi > lo)) continue;
            const float  k = sah::scale(lo, hi);
            sah::Box     bins[sah::BINS];
            int          cnt[sah::BINS] = {};
            for (auto& b : bins) b = sah::empty_box();
            const float* c = cen(d);
            for (size_t i = first; i < last; ++i) {
                const int32_t id = ids[i];
                const int     bi = sah::bin_of(c[id], lo, k);
                cnt[bi]++;
                spm::fold(bins[bi], bounds[id].lo, bounds[id].hi);
            }
            sah::sweep(d, cnt, bins, best);
        }
        const sah::Decision what = sah::decide(bb, static_cast<uint32_t>(n), static_cast<uint32_t>(max_leaf), best);
        const int           best_dim = best.dim, best_bin = best.bin;
        if (what == sah::MEDIAN) {
            // all centroids coincide: median split by index
            const size_t mid = first + n / 2;
            const uint32_t l = build(first, mid, depth + 1);
            const uint32_t r = build(mid, last, depth + 1);
            BvhNode& nd = nodes[me];
            for (int i = 0; i < 3; ++i) { nd.lo[i] = bb.lo[i]; nd.hi[i] = bb.hi[i]; }
            nd.a = l; nd.b = r;
            return me;
        }
        if (what == sah::LEAF) return make_leaf();
        const float  lo = cb.lo[best_dim], hi = cb.hi[best_dim];
        const float  k  = sah::scale(lo, hi);
        const float* c  = cen(best_dim);
        auto mid_it = std::stable_partition(ids.begin() + first, ids.begin() + last,
                                            [&](int32_t id) { return sah::goes_left(c[id], lo, k, best_bin); });
        size_t mid = static_cast<size_t>(mid_it - ids.begin());
        if (mid == first || mid == last) mid = first + n / 2;
        const uint32_t l = build(first, mid, depth + 1);
        const uint32_t r = build(mid, last, depth + 1);
        BvhNode& nd = nodes[me];
        for (int i = 0; i < 3; ++i) { nd.lo[i] = bb.lo[i]; nd.hi[i] = bb.hi[i]; }
        nd.a = l | (static_cast<uint32_t>(best_dim) << BVH_AXIS_SHIFT); // split axis: near-first order
        nd.b = r;
        return me;
    }
};
} // namespace

Bvh build_bvh_sah(const std::vector<PrimBounds>& bounds, int max_leaf)
{
    Bvh        out;
    SahBuilder b{ bounds, {}, {}, {}, {}, {}, max_leaf };
    const size_t n = bounds.size();
    b.ids.resize(n);
    b.cx.resize(n); b.cy.resize(n); b.cz.resize(n);
    for (size_t i = 0; i < n; ++i) {
        b.ids[i] = static_cast<int32_t>(i);
        b.cx[i]  = center_of(bounds[i], 0);
        b.cy[i]  = center_of(bounds[i], 1);
        b.cz[i]  = center_of(bounds[i], 2);
    }
    if (n >= (size_t(1) << BVH_AXIS_SHIFT)) throw std::runtime_error("too many primitives for the SAH BVH");
    if (n) b.build(0, n, 1);
    out.nodes      = std::move(b.nodes);
    out.prim_order = std::move(b.ids);
    out.max_depth  = b.max_depth;
    return out;
}

// The same tree level by level, the host restatement of the device SAH build
// (sp_sah_build.hip).  All open nodes of a level work on one ids array that stays stably
// partitioned; nodes are numbered breadth first, then subtree sizes bottom-up give the pre-order
// indices top-down (left = me + 1, right = me + 1 + nodes(left)).  What decides the tree -- node
// box, centroid box, bins -- enters only through differences, products and comparisons, so these
// are plain min / max reductions here, taken in reverse slot order on purpose: the sign of a zero
// extreme may differ from the recursive fold's and must not matter.  The stored box is the
// recursion's fold over the node's slots in the order they have when the node is split (its own
// partition comes after), which only differs from a min / max in the sign of a zero extreme.
Bvh build_bvh_sah_levels(const std::vector<PrimBounds>& bounds, int max_leaf)
{
    Bvh          out;
    const size_t n = bounds.size();
    if (n >= (size_t(1) << BVH_AXIS_SHIFT)) throw std::runtime_error("too many primitives for the SAH BVH");
    if (n == 0) return out;
    struct LNode {
        uint32_t first, count, left = 0, right = 0, axis = 0, size = 1, pre = 0;
        bool     leaf = true;
        float    lo[3] = { 0.0f, 0.0f, 0.0f }, hi[3] = { 0.0f, 0.0f, 0.0f };
    };
    std::vector<LNode>    bfs{ LNode{ 0u, (uint32_t)n } };
    std::vector<int32_t>  ids(n), next(n);
    for (size_t i = 0; i < n; ++i) ids[i] = (int32_t)i;
    std::vector<uint32_t> open{ 0u }, opened;
    auto cen = [&](int32_t id, int d) { return spm::centre(bounds[(size_t)id].lo[d], bounds[(size_t)id].hi[d]); };
    int  levels = 0;
    while (!open.empty()) {
        ++levels;
        next = ids; // slots outside a split keep their place
        opened.clear();
        for (const uint32_t me : open) {
            const uint32_t first = bfs[me].first, cnt_n = bfs[me].count, last = first + cnt_n;
            sah::Box bb = sah::empty_box(), cb = sah::empty_box();
            float    zlo[3] = { 0.0f, 0.0f, 0.0f }, zhi[3] = { 0.0f, 0.0f, 0.0f }; // the last slot's zero, per extreme
            bool     has_lo[3] = {}, has_hi[3] = {};
            for (uint32_t i = last; i-- > first;) {
                const PrimBounds& b = bounds[(size_t)ids[i]];
                for (int d = 0; d < 3; ++d) {
                    bb.lo[d] = lbvh::lower(bb.lo[d], b.lo[d]);
                    bb.hi[d] = lbvh::upper(bb.hi[d], b.hi[d]);
                    if (b.lo[d] == 0.0f && !has_lo[d]) { has_lo[d] = true; zlo[d] = b.lo[d]; }
                    if (b.hi[d] == 0.0f && !has_hi[d]) { has_hi[d] = true; zhi[d] = b.hi[d]; }
                    const float c = cen(ids[i], d);
                    cb.lo[d] = lbvh::lower(cb.lo[d], c);
                    cb.hi[d] = lbvh::upper(cb.hi[d], c);
                }
            }
            // the stored box: the recursion's fold in slot order keeps the later operand on a tie
            // between +0 and -0, so a zero extreme has the sign of the last slot that holds a zero
            for (int d = 0; d < 3; ++d) {
                if (bb.lo[d] == 0.0f) bb.lo[d] = zlo[d];
                if (bb.hi[d] == 0.0f) bb.hi[d] = zhi[d];
                bfs[me].lo[d] = bb.lo[d];
                bfs[me].hi[d] = bb.hi[d];
            }
            if (cnt_n <= 1) continue;
            sah::Best best;
            for (int d = 0; d < 3; ++d) {
                const float lo = cb.lo[d], hi = cb.hi[d];
                if (!(hi > lo)) continue;
                const float k = sah::scale(lo, hi);
                sah::Box    bins[sah::BINS];
                int         cnt[sah::BINS] = {};
                for (auto& b : bins) b = sah::empty_box();
                for (uint32_t i = last; i-- > first;) {
                    const PrimBounds& b  = bounds[(size_t)ids[i]];
                    const int         bi = sah::bin_of(cen(ids[i], d), lo, k);
                    cnt[bi]++;
                    for (int e = 0; e < 3; ++e) {
                        bins[bi].lo[e] = lbvh::lower(bins[bi].lo[e], b.lo[e]);
                        bins[bi].hi[e] = lbvh::upper(bins[bi].hi[e], b.hi[e]);
                    }
                }
                sah::sweep(d, cnt, bins, best);
            }
            const sah::Decision what = sah::decide(bb, cnt_n, (uint32_t)max_leaf, best);
            if (what == sah::LEAF) continue;
            uint32_t mid = first + cnt_n / 2, axis = 0;
            if (what == sah::SPLIT) {
                // stable partition as an exclusive scan of the predicate over the node's range
                const float lo = cb.lo[best.dim], k = sah::scale(cb.lo[best.dim], cb.hi[best.dim]);
                uint32_t    lefts = 0;
                for (uint32_t i = first; i < last; ++i) lefts += sah::goes_left(cen(ids[i], best.dim), lo, k, best.bin) ? 1u : 0u;
                axis = (uint32_t)best.dim;
                if (lefts != 0 && lefts != cnt_n) { // (else: the order stays, halved by index)
                    mid = first + lefts;
                    uint32_t l = first, r = mid;
                    for (uint32_t i = first; i < last; ++i)
                        next[sah::goes_left(cen(ids[i], best.dim), lo, k, best.bin) ? l++ : r++] = ids[i];
                }
            }
            const uint32_t l = (uint32_t)bfs.size();
            bfs[me].leaf  = false;
            bfs[me].axis  = axis;
            bfs[me].left  = l;
            bfs[me].right = l + 1;
            bfs.push_back(LNode{ first, mid - first });
            bfs.push_back(LNode{ mid, last - mid });
            opened.push_back(l);
            opened.push_back(l + 1);
        }
        ids.swap(next);
        open.swap(opened);
    }
    // subtree sizes bottom-up (children lie behind their parent), pre-order indices top-down
    for (size_t i = bfs.size(); i-- > 0;)
        if (!bfs[i].leaf) bfs[i].size = 1u + bfs[bfs[i].left].size + bfs[bfs[i].right].size;
    for (size_t i = 0; i < bfs.size(); ++i)
        if (!bfs[i].leaf) {
            bfs[bfs[i].left].pre  = bfs[i].pre + 1u;
            bfs[bfs[i].right].pre = bfs[i].pre + 1u + bfs[bfs[i].left].size;
        }
    out.nodes.assign(bfs.size(), BvhNode{});
    for (const LNode& b : bfs) {
        BvhNode& nd = out.nodes[b.pre];
        for (int d = 0; d < 3; ++d) { nd.lo[d] = b.lo[d]; nd.hi[d] = b.hi[d]; }
        if (b.leaf) {
            nd.a = b.first;
            nd.b = b.count | BVH_LEAF;
        } else {
            nd.a = bfs[b.left].pre | b.axis << BVH_AXIS_SHIFT;
            nd.b = bfs[b.right].pre;
        }
    }
    out.prim_order = std::move(ids);
    out.max_depth  = levels;
    return out;
}

// ------------------------------------------------------------------------------ linear BVH
// The device builder's algorithm (sp_build.hip) step by step on the host: the
// arithmetic is sp_lbvh.h on both sides, the sort is stable on both sides, and the box merges
// keep one operand order, so the two trees are equal bit for bit.
int bvh_walk_depth(const std::vector<BvhNode>& nodes)
{
    if (nodes.empty()) return 0;
    int                                     depth = 0;
    size_t                                  seen  = 0;
    std::vector<std::pair<uint32_t, int>>   stack{ { 0u, 1 } };
    while (!stack.empty()) {
        const auto [i, d] = stack.back();
        stack.pop_back();
        if (i >= nodes.size() || ++seen > nodes.size()) throw std::runtime_error("BVH links do not form a tree");
        depth = std::max(depth, d);
        if (nodes[i].b & BVH_LEAF) continue;
        stack.push_back({ nodes[i].b, d + 1 });
        stack.push_back({ nodes[i].a & BVH_CHILD_MASK, d + 1 });
    }
    return depth;
}

void lbvh_fit_boxes(Bvh& bvh, const std::vector<PrimBounds>& bounds)
{
    std::vector<BvhNode>& nodes = bvh.nodes;
    if (nodes.empty()) return;
    // parents before children, then backwards
    std::vector<uint32_t> order;
    order.reserve(nodes.size());
    std::vector<uint32_t> stack{ 0u };
    while (!stack.empty()) {
        const uint32_t i = stack.back();
        stack.pop_back();
        if (i >= nodes.size() || order.size() >= nodes.size()) throw std::runtime_error("BVH links do not form a tree");
        order.push_back(i);
        if (nodes[i].b & BVH_LEAF) continue;
        stack.push_back(nodes[i].b);
        stack.push_back(nodes[i].a & BVH_CHILD_MASK);
    }
    for (size_t k = order.size(); k-- > 0;) {
        BvhNode& nd = nodes[order[k]];
        if (nd.b & BVH_LEAF) {
            Box bb = empty_box();
            for (uint32_t s = 0; s < (nd.b & ~BVH_LEAF); ++s) bb = merge(bb, bounds[(size_t)bvh.prim_order[nd.a + s]]);
            for (int i = 0; i < 3; ++i) { nd.lo[i] = bb.lo[i]; nd.hi[i] = bb.hi[i]; }
        } else {
            const BvhNode& l = nodes[nd.a & BVH_CHILD_MASK];
            const BvhNode& r = nodes[nd.b];
            for (int i = 0; i < 3; ++i) {
                nd.lo[i] = spm::sse_min(l.lo[i], r.lo[i]);
                nd.hi[i] = spm::sse_max(l.hi[i], r.hi[i]);
            }
        }
    }
}

Bvh build_bvh_lbvh(const std::vector<PrimBounds>& bounds, int max_leaf)
{
    Bvh          out;
    const size_t n = bounds.size();
    if (n >= (size_t(1) << BVH_AXIS_SHIFT)) throw std::runtime_error("too many primitives for the linear BVH");
    if (max_leaf < 1 || max_leaf > 4) throw std::runtime_error("linear BVH: leaf size must be 1..4");
    if (n == 0) return out;
    // centroid bounds, cells, codes
    float cb_lo[3] = { INFINITY, INFINITY, INFINITY }, cb_hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (const PrimBounds& b : bounds)
        for (int d = 0; d < 3; ++d) {
            const float c = spm::centre(b.lo[d], b.hi[d]);
            cb_lo[d]      = lbvh::lower(cb_lo[d], c);
            cb_hi[d]      = lbvh::upper(cb_hi[d], c);
        }
    std::vector<uint64_t> key(n);
    for (size_t i = 0; i < n; ++i) {
        uint32_t q[3];
        for (int d = 0; d < 3; ++d) q[d] = lbvh::cell(spm::centre(bounds[i].lo[d], bounds[i].hi[d]), cb_lo[d], cb_hi[d]);
        key[i] = lbvh::code(q[0], q[1], q[2]);
    }
    // stable sort of (code, id) by code
    out.prim_order.resize(n);
    for (size_t i = 0; i < n; ++i) out.prim_order[i] = (int32_t)i;
    std::stable_sort(out.prim_order.begin(), out.prim_order.end(), [&](int32_t a, int32_t b) { return key[(size_t)a] < key[(size_t)b]; });
    std::vector<uint64_t> codes(n);
    for (size_t i = 0; i < n; ++i) codes[i] = key[(size_t)out.prim_order[i]];
    // candidates: internal nodes 0..n-2, then single primitives; a child is kept when its parent
    // covers more than max_leaf positions, and a kept node covering at most max_leaf is a leaf
    const uint32_t           un = (uint32_t)n, total = 2 * un - 1;
    std::vector<lbvh::Range> rng(n - 1);
    std::vector<uint32_t>    keep(total, 0u), index(total);
    // (ranges only shrink downwards, so "the parent covers more" holds for every ancestor too)
    keep[0] = 1; // the root: internal node 0, or the only primitive
    for (uint32_t i = 0; i + 1 < un; ++i) {
        rng[i] = lbvh::node_range(codes.data(), (int64_t)n, i);
        const uint32_t kept = (rng[i].last - rng[i].first + 1 > (uint32_t)max_leaf) ? 1u : 0u;
        keep[lbvh::left_cand(rng[i], un)]  = kept;
        keep[lbvh::right_cand(rng[i], un)] = kept;
    }
    uint32_t m = 0;
    for (uint32_t c = 0; c < total; ++c) { index[c] = m; m += keep[c]; }
    out.nodes.assign(m, BvhNode{});
    for (uint32_t c = 0; c < total; ++c) {
        if (!keep[c]) continue;
        BvhNode& nd = out.nodes[index[c]];
        if (c < un - 1 && rng[c].last - rng[c].first + 1 > (uint32_t)max_leaf) {
            nd.a = index[lbvh::left_cand(rng[c], un)] | rng[c].axis << BVH_AXIS_SHIFT;
            nd.b = index[lbvh::right_cand(rng[c], un)];
        } else {
            const uint32_t first = c < un - 1 ? rng[c].first : c - (un - 1);
            const uint32_t count = c < un - 1 ? rng[c].last - rng[c].first + 1 : 1u;
            nd.a = first;
            nd.b = count | BVH_LEAF;
        }
    }
    lbvh_fit_boxes(out, bounds);
    out.max_depth = bvh_walk_depth(out.nodes);
    return out;
}

// ------------------------------------------------------------------------------ checker
BvhCheck check_bvh(const Bvh& bvh, const std::vector<PrimBounds>& bounds, int max_leaf)
{
    BvhCheck   r;
    const auto& nodes = bvh.nodes;
    r.nodes = (int64_t)nodes.size();
    r.slots = (int64_t)bvh.prim_order.size();
    auto bad = [&](int kind, int64_t node) {
        if (r.errors++ == 0) { r.first_error_kind = kind; r.first_error_node = node; }
    };
    uint64_t h = 0xcbf29ce484222325ull;
    auto fnv = [&](const void* p, size_t bytes) {
        const unsigned char* c = static_cast<const unsigned char*>(p);
        for (size_t i = 0; i < bytes; ++i) { h ^= c[i]; h *= 0x100000001b3ull; }
    };
    fnv(nodes.data(), nodes.size() * sizeof(BvhNode));
    fnv(bvh.prim_order.data(), bvh.prim_order.size() * sizeof(int32_t));
    r.hash = h;
    // prim_order: a permutation of the bounded primitives
    const size_t np = bounds.size();
    bool         order_ok = bvh.prim_order.size() == np;
    {
        std::vector<uint8_t> seen(np, 0);
        for (size_t s = 0; s < bvh.prim_order.size(); ++s) {
            const int32_t p = bvh.prim_order[s];
            if (p < 0 || (size_t)p >= np || seen[(size_t)p]++) { bad(BVH_ERR_PRIM_ORDER, (int64_t)s); order_ok = false; }
        }
        if (bvh.prim_order.size() != np) bad(BVH_ERR_PRIM_ORDER, -1);
    }
    if (nodes.empty()) {
        if (np != 0) bad(BVH_ERR_SLOT_PARTITION, -1);
        if (bvh.max_depth != 0) bad(BVH_ERR_DEPTH, -1);
        return r;
    }
    auto outside = [](const float* lo, const float* hi, const BvhNode& n) {
        for (int d = 0; d < 3; ++d)
            if (lo[d] < n.lo[d] || hi[d] > n.hi[d]) return true;
        return false;
    };
    std::vector<uint8_t>                  visited(nodes.size(), 0), covered(bvh.prim_order.size(), 0);
    std::vector<std::pair<uint32_t, int>> stack{ { 0u, 1 } };
    while (!stack.empty()) {
        const auto [i, depth] = stack.back();
        stack.pop_back();
        if (visited[i]) { bad(BVH_ERR_VISITED_TWICE, i); continue; }
        visited[i] = 1;
        r.depth    = std::max(r.depth, depth);
        const BvhNode& nd = nodes[i];
        if (nd.b & BVH_LEAF) {
            const uint32_t cnt = nd.b & ~BVH_LEAF;
            ++r.leaves;
            r.max_leaf = std::max<int>(r.max_leaf, (int)std::min<uint32_t>(cnt, 0x7fffffffu));
            if (cnt < 1 || (max_leaf > 0 && (cnt > 7 || cnt > (uint32_t)max_leaf))) bad(BVH_ERR_LEAF_COUNT, i);
            if ((uint64_t)nd.a + cnt > covered.size()) { bad(BVH_ERR_SLOT_PARTITION, i); continue; }
            for (uint32_t s = 0; s < cnt; ++s) {
                if (covered[nd.a + s]++) bad(BVH_ERR_SLOT_PARTITION, i);
                const int32_t p = bvh.prim_order[nd.a + s];
                if (order_ok && outside(bounds[(size_t)p].lo, bounds[(size_t)p].hi, nd)) bad(BVH_ERR_BOX, i);
            }
            continue;
        }
        const uint32_t kids[2] = { nd.a & BVH_CHILD_MASK, nd.b };
        for (int k = 1; k >= 0; --k) {
            if (kids[k] >= nodes.size()) { bad(BVH_ERR_CHILD_RANGE, i); continue; }
            if (outside(nodes[kids[k]].lo, nodes[kids[k]].hi, nd)) bad(BVH_ERR_BOX, i);
            stack.push_back({ kids[k], depth + 1 });
        }
    }
    for (size_t i = 0; i < nodes.size(); ++i)
        if (!visited[i]) bad(BVH_ERR_UNREACHABLE, (int64_t)i);
    for (size_t s = 0; s < covered.size(); ++s)
        if (!covered[s]) bad(BVH_ERR_SLOT_PARTITION, -1); // (a slot covered twice is counted above)
    if (r.depth != bvh.max_depth) bad(BVH_ERR_DEPTH, -1);
    return r;
}

// ---------------------------------------------------------------- 8-wide collapse
// The per-node work -- which children a wide node takes, their octant slots, the quantisation --
// is spw::collapse (sp_wide.h), shared with the level-wise form below and the device finish.
namespace {

struct WideBuilder {
    const Bvh& b;
    WideBvh&   out;

    void emit(uint32_t wi, uint32_t bi, int depth)
    {
        out.depth = std::max(out.depth, depth);
        spw::Collapsed c;
        const int      e = spw::collapse(b.nodes.data(), (uint32_t)b.nodes.size(), bi, c);
        if (e != spw::OK) throw std::runtime_error(spw::error_text(e));
        // inner child in slot s is node child_base + s (slots taken by leaves or empty leave holes)
        const uint32_t child_base = (uint32_t)(out.words.size() / 20);
        out.words.resize(out.words.size() + 20 * (size_t)c.span);
        const uint32_t leaf_base = (uint32_t)out.slot_of.size();
        out.slot_of.resize(out.slot_of.size() + c.own);
        spw::write_slots(b.nodes.data(), c, leaf_base, out.slot_of.data());
        uint32_t* w = &out.words[(size_t)wi * 20];
        std::memcpy(w, c.w, sizeof c.w);
        w[4] = child_base;
        w[5] = leaf_base;
        for (int s = 0; s < 8; ++s)
            if ((c.imask >> s) & 1u) emit(child_base + (uint32_t)s, c.kid[s], depth + 1);
    }
};

} // namespace

WideBvh build_wide(const Bvh& bvh)
{
    WideBvh out;
    if (bvh.nodes.empty()) return out;
    out.words.resize(20);
    WideBuilder wb{ bvh, out };
    wb.emit(0, 0, 1);
    if (out.words.size() / 20 >= (1u << 24)) throw std::runtime_error("wide BVH: more than 2^24 nodes");
    if (std::getenv("SP_WIDE_STATS"))
        std::fprintf(stderr, "wide BVH: %zu node records, %zu leaf slots, depth %d\n", out.words.size() / 20, out.slot_of.size(), out.depth);
    return out;
}

// ------------------------------------------------------------------ level-wise collapse
// build_wide numbers records (child_base) and slots (leaf_base) with running counters in
// pre-order.  Both have a closed form in the subtree sums N(v) = span(v) + sum N(c) and
// L(v) = own(v) + sum L(c) over the inner children c in slot order: the k-th of them has
// child_base(v) + span(v) + sum_{j<k} N(c_j) and leaf_base(v) + own(v) + sum_{j<k} L(c_j), and
// its record at child_base(v) + slot.  So the levels can be worked one after another.
WideBvh build_wide_levels(const Bvh& bvh)
{
    WideBvh out;
    if (bvh.nodes.empty()) return out;
    struct Item {
        uint32_t root, record;      // binary root; final record index (set top-down)
        uint32_t first_child;       // index of its first inner child in the next level's list
        uint32_t n_sub, l_sub;      // N, L
        uint32_t child_base, leaf_base;
        spw::Collapsed c;
    };
    const BvhNode*                 nodes = bvh.nodes.data();
    std::vector<std::vector<Item>> levels;
    // 1. top-down: collapse; count, exclusive scan, scatter
    {
        Item root{};
        root.root = 0;
        levels.push_back({ root });
    }
    size_t collapsed = 0;
    for (size_t l = 0;; ++l) {
        std::vector<Item>& cur = levels[l];
        std::vector<uint32_t> count(cur.size());
        for (size_t i = 0; i < cur.size(); ++i) {
            const int e = spw::collapse(nodes, (uint32_t)bvh.nodes.size(), cur[i].root, cur[i].c);
            if (e != spw::OK) throw std::runtime_error(spw::error_text(e));
            count[i] = (uint32_t)__builtin_popcount(cur[i].c.imask);
        }
        collapsed += cur.size();
        if (collapsed > bvh.nodes.size()) throw std::runtime_error(spw::error_text(spw::ERR_LINKS));
        uint32_t total = 0;
        for (size_t i = 0; i < cur.size(); ++i) { cur[i].first_child = total; total += count[i]; }
        if (total == 0) break;
        if (levels.size() >= (size_t)spw::MAX_LEVELS) throw std::runtime_error(spw::error_text(spw::ERR_LEVELS));
        std::vector<Item> next(total, Item{});
        for (size_t i = 0; i < cur.size(); ++i) {
            uint32_t k = cur[i].first_child;
            for (int s = 0; s < 8; ++s)
                if ((cur[i].c.imask >> s) & 1u) next[k++].root = cur[i].c.kid[s];
        }
        levels.push_back(std::move(next)); // (cur is dangling from here)
    }
    out.depth = (int)levels.size();
    // 2. bottom-up: subtree sums
    for (size_t l = levels.size(); l-- > 0;)
        for (Item& v : levels[l]) {
            uint64_t n = (uint64_t)v.c.span, ls = v.c.own;
            uint32_t k = v.first_child;
            for (int s = 0; s < 8; ++s)
                if ((v.c.imask >> s) & 1u) { n += levels[l + 1][k].n_sub; ls += levels[l + 1][k].l_sub; ++k; }
            if (n + 1 >= spw::MAX_RECORDS) throw std::runtime_error(spw::error_text(spw::ERR_RECORDS));
            v.n_sub = (uint32_t)n;
            v.l_sub = (uint32_t)ls;
        }
    // 3. top-down: bases
    levels[0][0].record     = 0;
    levels[0][0].child_base = 1;
    levels[0][0].leaf_base  = 0;
    for (size_t l = 0; l + 1 < levels.size(); ++l)
        for (const Item& v : levels[l]) {
            uint32_t cb = v.child_base + (uint32_t)v.c.span, lb = v.leaf_base + v.c.own, k = v.first_child;
            for (int s = 0; s < 8; ++s) {
                if (!((v.c.imask >> s) & 1u)) continue;
                Item& c      = levels[l + 1][k++];
                c.record     = v.child_base + (uint32_t)s;
                c.child_base = cb;
                c.leaf_base  = lb;
                cb += c.n_sub;
                lb += c.l_sub;
            }
        }
    // 4. records and slots at their final places; holes stay zero
    out.words.assign(20 * (size_t)(1u + levels[0][0].n_sub), 0u);
    out.slot_of.assign(levels[0][0].l_sub, 0);
    for (const auto& level : levels)
        for (const Item& v : level) {
            uint32_t* w = &out.words[20 * (size_t)v.record];
            std::memcpy(w, v.c.w, sizeof v.c.w);
            w[4] = v.child_base;
            w[5] = v.leaf_base;
            spw::write_slots(nodes, v.c, v.leaf_base, out.slot_of.data());
        }
    return out;
}

// ------------------------------------------------------------------------- wide refit
// Records sit behind their parents (child_base is taken from a running count in both collapses),
// so the array walked backwards meets every child before its parent.
void refit_wide(WideBvh& wide, const std::vector<PrimBounds>& slot_bounds)
{
    std::vector<uint32_t>& W    = wide.words;
    const size_t           nrec = W.size() / 20, nslots = slot_bounds.size();
    std::vector<spr::Box>  exact(nrec, spr::empty_box());
    for (size_t r = nrec; r-- > 0;) {
        uint32_t*      w     = &W[20 * r];
        const uint32_t imask = spr::rec_imask(w), occupied = spr::rec_occupied(w);
        spr::Box       slot[8];
        for (int s = 0; s < 8; ++s) {
            slot[s] = spr::empty_box();
            if ((imask >> s) & 1u) {
                const uint64_t c = (uint64_t)w[4] + (uint32_t)s;
                if (c <= r || c >= nrec) throw std::runtime_error(spw::error_text(spw::ERR_LINKS));
                slot[s] = exact[c];
                continue;
            }
            const uint32_t meta = spr::rec_meta(w, s), cnt = meta >> 5, off = meta & 31u;
            if ((uint64_t)w[5] + off + cnt > nslots) throw std::runtime_error(spw::error_text(spw::ERR_LINKS));
            for (uint32_t j = 0; j < cnt; ++j) {
                const PrimBounds& b = slot_bounds[(size_t)w[5] + off + j];
                spr::Box          pb;
                for (int a = 0; a < 3; ++a) { pb.lo[a] = b.lo[a]; pb.hi[a] = b.hi[a]; }
                spr::fold(slot[s], pb);
            }
        }
        const int e = spr::refit_record(w, slot, occupied, exact[r]);
        if (e != spw::OK) throw std::runtime_error(spw::error_text(e));
    }
}

// ------------------------------------------------------------------------- wide checker
uint64_t fnv1a64(const void* p, size_t bytes, uint64_t h)
{
    const unsigned char* c = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < bytes; ++i) { h ^= c[i]; h *= 0x100000001b3ull; }
    return h;
}

WideCheck check_wide(const WideBvh& wide, const std::vector<int32_t>& prim_order, const std::vector<PrimBounds>& bounds)
{
    WideCheck r;
    const std::vector<uint32_t>& W = wide.words;
    const size_t nrec = W.size() / 20, nslots = wide.slot_of.size();
    r.records = (int64_t)nrec;
    r.slots   = (int64_t)nslots;
    auto bad = [&](int kind, int64_t node) {
        if (r.errors++ == 0) { r.first_error_kind = kind; r.first_error_node = node; }
    };
    if (W.empty()) {
        if (nslots != 0) bad(WIDE_ERR_SLOT_PARTITION, -1);
        if (wide.depth != 0) bad(WIDE_ERR_DEPTH, -1);
        return r;
    }
    r.hash_nodes = fnv1a64(W.data(), W.size() * 4);
    // the wide slots name every binary slot once
    bool slots_ok = nslots == prim_order.size();
    if (!slots_ok) bad(WIDE_ERR_RECORDS, -1);
    {
        std::vector<uint8_t> seen(prim_order.size(), 0);
        for (size_t i = 0; i < nslots; ++i) {
            const int32_t b = wide.slot_of[i];
            if (b < 0 || (size_t)b >= seen.size() || seen[(size_t)b]++) { bad(WIDE_ERR_RECORDS, (int64_t)i); slots_ok = false; }
        }
    }
    // 0 unseen, 1 reached, 2 inside a reached node's span
    std::vector<uint8_t> state(nrec, 0), covered(nslots, 0);
    state[0] = 2;
    struct Frame {
        uint32_t rec;
        int      depth, slot;   // next slot to look at
        int      from;          // the parent frame's slot this one hangs in
        Box      acc;           // union of what lies beneath the slot being worked
    };
    auto decoded_outside = [&](const uint32_t* w, int s, const Box& u) {
        for (int a = 0; a < 3; ++a) {
            float origin, step;
            std::memcpy(&origin, &w[a], 4);
            const uint32_t sb = ((w[3] >> (8 * a)) & 0xffu) << 23;
            std::memcpy(&step, &sb, 4);
            const uint32_t ql = (w[8 + 2 * a + s / 4] >> (8 * (s % 4))) & 0xffu;
            const uint32_t qh = (w[8 + 2 * (3 + a) + s / 4] >> (8 * (s % 4))) & 0xffu;
            const float    dlo = std::fma((float)ql, step, origin), dhi = std::fma((float)qh, step, origin);
            if (u.lo[a] < dlo || u.hi[a] > dhi) return true;
        }
        return false;
    };
    auto merge_box = [](Box& into, const Box& b) {
        for (int a = 0; a < 3; ++a) {
            into.lo[a] = spm::sse_min(into.lo[a], b.lo[a]);
            into.hi[a] = spm::sse_max(into.hi[a], b.hi[a]);
        }
    };
    std::vector<Frame> stack;
    std::vector<Box>   total; // per frame: union of the whole node
    auto enter = [&](uint32_t rec, int depth, int from) {
        stack.push_back(Frame{ rec, depth, 0, from, empty_box() });
        total.push_back(empty_box());
        r.depth = std::max(r.depth, depth);
        const uint32_t* w = &W[20 * (size_t)rec];
        bool            zero = true;
        for (int i = 0; i < 20; ++i) zero = zero && w[i] == 0u;
        if (zero) bad(WIDE_ERR_HOLE, rec); // an imask names a hole
        const uint32_t imask = w[3] >> 24;
        int            span  = 0;
        for (int s = 0; s < 8; ++s)
            if ((imask >> s) & 1u) span = s + 1;
        for (int s = 0; s < span; ++s)
            if ((uint64_t)w[4] + (uint32_t)s < nrec && state[w[4] + (uint32_t)s] == 0) state[w[4] + (uint32_t)s] = 2;
    };
    state[0] = 1;
    enter(0, 1, -1);
    while (!stack.empty()) {
        Frame&          f = stack.back();
        const uint32_t* w = &W[20 * (size_t)f.rec];
        if (f.slot == 8) { // done: hand the union up
            const Box  mine = total.back();
            const int  from = f.from;
            stack.pop_back();
            total.pop_back();
            if (!stack.empty()) {
                const uint32_t* pw = &W[20 * (size_t)stack.back().rec];
                if (decoded_outside(pw, from, mine)) bad(WIDE_ERR_BOX, stack.back().rec);
                merge_box(total.back(), mine);
            }
            continue;
        }
        const int      s     = f.slot++;
        const uint32_t imask = w[3] >> 24;
        const uint32_t meta  = (w[6 + s / 4] >> (8 * (s % 4))) & 0xffu;
        if (s == 0 && ((w[3] & 0xffu) == 0xffu || ((w[3] >> 8) & 0xffu) == 0xffu || ((w[3] >> 16) & 0xffu) == 0xffu)) bad(WIDE_ERR_QUANT, f.rec);
        if (((imask >> s) & 1u) || meta != 0)
            for (int a = 0; a < 3; ++a)
                if (((w[8 + 2 * a + s / 4] >> (8 * (s % 4))) & 0xffu) > ((w[14 + 2 * a + s / 4] >> (8 * (s % 4))) & 0xffu)) { bad(WIDE_ERR_QUANT, f.rec); break; }
        if ((imask >> s) & 1u) {
            const uint64_t c = (uint64_t)w[4] + (uint32_t)s;
            if (c >= nrec) { bad(WIDE_ERR_CHILD_RANGE, f.rec); continue; }
            if (state[c] == 1) { bad(WIDE_ERR_VISITED_TWICE, (int64_t)c); continue; }
            state[c] = 1;
            if (meta != 0) bad(WIDE_ERR_META, f.rec);
            enter((uint32_t)c, f.depth + 1, s); // (f is dangling from here)
            continue;
        }
        if (meta == 0) continue; // empty slot
        const uint32_t cnt = meta >> 5, off = meta & 31u; // (cnt <= 7 and off <= 31 by construction of the byte)
        if (cnt == 0) { bad(WIDE_ERR_META, f.rec); continue; }
        if ((uint64_t)w[5] + off + cnt > nslots) { bad(WIDE_ERR_SLOT_PARTITION, f.rec); continue; }
        Box u = empty_box();
        for (uint32_t j = 0; j < cnt; ++j) {
            const size_t ws = (size_t)w[5] + off + j;
            if (covered[ws]++) bad(WIDE_ERR_SLOT_PARTITION, f.rec);
            if (!slots_ok) continue;
            const int32_t p = prim_order[(size_t)wide.slot_of[ws]];
            if (p < 0 || (size_t)p >= bounds.size()) continue; // (the binary checker reports the order)
            u = merge(u, bounds[(size_t)p]);
        }
        if (slots_ok && decoded_outside(w, s, u)) bad(WIDE_ERR_BOX, f.rec);
        merge_box(total.back(), u);
    }
    for (size_t i = 0; i < nrec; ++i) {
        if (state[i] == 1) continue;
        if (state[i] == 0) { bad(WIDE_ERR_UNREACHABLE, (int64_t)i); continue; }
        ++r.holes;
        for (int k = 0; k < 20; ++k)
            if (W[20 * i + (size_t)k] != 0u) { bad(WIDE_ERR_HOLE, (int64_t)i); break; }
    }
    for (size_t s = 0; s < nslots; ++s)
        if (!covered[s]) bad(WIDE_ERR_SLOT_PARTITION, -1);
    if (r.depth != wide.depth) bad(WIDE_ERR_DEPTH, -1);
    return r;
}

} // namespace sph
