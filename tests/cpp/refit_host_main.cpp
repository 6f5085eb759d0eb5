// refit_host_main.cpp -- the host restatement of the refit (sp_bvh.cpp lbvh_fit_boxes, refit_wide;
// DESIGN.md section 21) and the two structural checkers on constructed bounds, as a stand-alone
// program so that it can run under -fsanitize=address,undefined (tests/test_refit_host.py compiles
// and runs it).  Per set, builder and leaf size: build at pose A, refit the same arrays to pose B
// (every box is stale), check against B's bounds, refit back to A and compare with a refit of the
// untouched build to A.  Then a stale box is planted in each tree and the checkers must count it.
// Exit status 0 only when every step holds.
#include "../../simplepath_amd/csrc/host/sp_host.hpp"
#include "../../simplepath_amd/csrc/common/sp_refit.h"

#include <cmath>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

using sph::PrimBounds;

static PrimBounds box(float x, float y, float z, float r)
{
    return PrimBounds{ { x - r, y - r, z - r }, { x + r, y + r, z + r } };
}

static std::vector<PrimBounds> random_set(size_t n, unsigned seed)
{
    std::mt19937                          g(seed);
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    std::vector<PrimBounds>               v;
    for (size_t i = 0; i < n; ++i) v.push_back(box(u(g), u(g), u(g), 0.01f + 0.02f * std::fabs(u(g))));
    return v;
}

// pose B: every box somewhere else, some shrunk to a point, one pushed far out
static std::vector<PrimBounds> moved(const std::vector<PrimBounds>& a, unsigned seed)
{
    std::mt19937                          g(seed);
    std::uniform_real_distribution<float> u(-0.5f, 0.5f);
    std::vector<PrimBounds>               b = a;
    for (size_t i = 0; i < b.size(); ++i) {
        const float d[3] = { 0.37f + u(g), -0.21f + u(g), 0.11f + u(g) };
        for (int k = 0; k < 3; ++k) { b[i].lo[k] += d[k]; b[i].hi[k] += d[k]; }
        if (i % 3 == 0)
            for (int k = 0; k < 3; ++k) b[i].hi[k] = b[i].lo[k];
    }
    if (!b.empty())
        for (int k = 0; k < 3; ++k) { b[0].lo[k] += 1000.0f; b[0].hi[k] += 1000.0f; }
    return b;
}

struct Trees {
    sph::Bvh     bvh;
    sph::WideBvh wide;
};

// sp_capi.hip refit_host on bounds alone: the binary boxes, then the wide records from the bounds
// in wide-slot order
static void refit(Trees& t, const std::vector<PrimBounds>& bounds)
{
    sph::lbvh_fit_boxes(t.bvh, bounds);
    std::vector<PrimBounds> by_wide_slot(t.wide.slot_of.size());
    for (size_t i = 0; i < by_wide_slot.size(); ++i) by_wide_slot[i] = bounds[(size_t)t.bvh.prim_order[(size_t)t.wide.slot_of[i]]];
    sph::refit_wide(t.wide, by_wide_slot);
}

static bool same_nodes(const sph::Bvh& a, const sph::Bvh& b)
{
    return sph::fnv1a64(a.nodes.data(), a.nodes.size() * sizeof(sph::BvhNode)) ==
               sph::fnv1a64(b.nodes.data(), b.nodes.size() * sizeof(sph::BvhNode)) &&
           a.prim_order == b.prim_order;
}

static int failures = 0;

static void run_tree(const std::string& name, const char* builder, int leaf, const sph::Bvh& built, const std::vector<PrimBounds>& a,
                     const std::vector<PrimBounds>& b)
{
    Trees first{ built, sph::build_wide(built) };
    Trees t = first, a_to_a = first;
    refit(a_to_a, a);
    // a linear BVH's boxes are lbvh_fit_boxes' own: refitting to the same bounds changes no byte of it
    const bool null_ok = std::string(builder) != "lbvh" || same_nodes(a_to_a.bvh, first.bvh);
    refit(t, b);
    const sph::BvhCheck  cb = sph::check_bvh(t.bvh, b, leaf);
    const sph::WideCheck cw = sph::check_wide(t.wide, t.bvh.prim_order, b);
    const bool           stale = a.empty() || sph::check_bvh(first.bvh, b, leaf).errors > 0; // the old boxes do not hold B
    refit(t, a);
    const bool back = same_nodes(t.bvh, a_to_a.bvh) && t.wide.words == a_to_a.wide.words && t.wide.slot_of == first.wide.slot_of &&
                      t.wide.depth == first.wide.depth;
    const sph::WideCheck ca = sph::check_wide(t.wide, t.bvh.prim_order, a);
    const bool           ok = null_ok && cb.errors == 0 && cw.errors == 0 && stale && back && ca.errors == 0 &&
                    sph::check_bvh(t.bvh, a, leaf).errors == 0 && cw.records == (int64_t)first.wide.words.size() / 20;
    std::printf("refit %-12s %-5s leaf %d: nodes %lld records %lld bvh errors %lld wide errors %lld back %d null %d %s\n", name.c_str(),
                builder, leaf, (long long)cb.nodes, (long long)cw.records, (long long)cb.errors, (long long)cw.errors, (int)back,
                (int)null_ok, ok ? "ok" : "FAILED");
    failures += !ok;
}

static void run(const std::string& name, const std::vector<PrimBounds>& a, unsigned seed)
{
    const std::vector<PrimBounds> b = moved(a, seed);
    for (int leaf : { 1, 2, 4 }) {
        run_tree(name, "lbvh", leaf, sph::build_bvh_lbvh(a, leaf), a, b);
        run_tree(name, "sah", leaf, sph::build_bvh_sah(a, leaf), a, b);
    }
}

int main()
{
    for (size_t n : { 0, 1, 2, 8, 9, 64, 65, 257, 1025 }) run("random" + std::to_string(n), random_set(n, 3u + (unsigned)n), 40u + (unsigned)n);
    run("identical37", std::vector<PrimBounds>(37, box(0.1f, 0.2f, 0.3f, 0.5f)), 7);
    run("points", std::vector<PrimBounds>(20, box(0.25f, -0.5f, 0.125f, 0.0f)), 8);
    {
        // the checkers on a refit that missed one box: refit everything to B, then put one old box back
        const std::vector<PrimBounds> a = random_set(300, 9), b = moved(a, 10);
        const sph::Bvh                built = sph::build_bvh_sah(a, 2);
        Trees                         old{ built, sph::build_wide(built) };
        Trees                         t = old;
        refit(t, b);
        if (sph::check_bvh(t.bvh, b, 2).errors != 0 || sph::check_wide(t.wide, t.bvh.prim_order, b).errors != 0 ||
            t.wide.words.size() / 20 < 10) {
            std::printf("planted: the base trees are not fit for the test\n");
            ++failures;
        }
        {
            Trees d = t;
            // the leaf that holds primitive 0, which moved farthest
            size_t leaf = 0;
            for (size_t i = 0; i < d.bvh.nodes.size(); ++i) {
                const sph::BvhNode& n = d.bvh.nodes[i];
                if (!(n.b & sph::BVH_LEAF)) continue;
                for (uint32_t s = 0; s < (n.b & ~sph::BVH_LEAF); ++s)
                    if (d.bvh.prim_order[n.a + s] == 0) leaf = i;
            }
            for (int k = 0; k < 3; ++k) { d.bvh.nodes[leaf].lo[k] = old.bvh.nodes[leaf].lo[k]; d.bvh.nodes[leaf].hi[k] = old.bvh.nodes[leaf].hi[k]; }
            const sph::BvhCheck c  = sph::check_bvh(d.bvh, b, 2);
            const bool          ok = c.errors > 0 && c.first_error_kind == sph::BVH_ERR_BOX;
            std::printf("planted stale binary box: errors %lld kind %d node %lld %s\n", (long long)c.errors, c.first_error_kind,
                        (long long)c.first_error_node, ok ? "ok" : "FAILED");
            failures += !ok;
        }
        {
            Trees d = t;
            // the root record as it was before the refit: its grid does not reach the moved primitives
            for (int k = 0; k < 20; ++k) d.wide.words[(size_t)k] = old.wide.words[(size_t)k];
            const sph::WideCheck c  = sph::check_wide(d.wide, d.bvh.prim_order, b);
            const bool           ok = c.errors > 0 && c.first_error_kind == sph::WIDE_ERR_BOX;
            std::printf("planted stale wide box: errors %lld kind %d node %lld %s\n", (long long)c.errors, c.first_error_kind,
                        (long long)c.first_error_node, ok ? "ok" : "FAILED");
            failures += !ok;
        }
    }
    {
        // a child link that points past the records is refused, not followed
        const std::vector<PrimBounds> a = random_set(100, 11);
        const sph::Bvh                built = sph::build_bvh_sah(a, 1);
        Trees                         t{ built, sph::build_wide(built) };
        t.wide.words[4] = (uint32_t)(t.wide.words.size() / 20);
        bool threw = false;
        try {
            refit(t, a);
        } catch (const std::exception&) {
            threw = true;
        }
        std::printf("refused child link: %s\n", threw ? "ok" : "FAILED");
        failures += !threw;
    }
    std::printf("%d failing\n", failures);
    return failures ? 1 : 0;
}
