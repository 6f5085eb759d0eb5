// lbvh_host_main.cpp -- the host BVH builders and the checker (sp_bvh.cpp) on constructed bounds,
// as a stand-alone program so that it can run under -fsanitize=address,undefined
// (tests/test_device_build_host.py compiles and runs it).  Prints one line per case and a summary;
// exit status 0 only when every tree passes the checker.
#include "../../simplepath_amd/csrc/host/sp_host.hpp"

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

static int failures = 0;

static void run(const std::string& name, const std::vector<PrimBounds>& b)
{
    for (int leaf = 1; leaf <= 4; ++leaf) {
        const sph::Bvh      t  = sph::build_bvh_lbvh(b, leaf);
        const sph::BvhCheck c  = sph::check_bvh(t, b, leaf);
        const sph::BvhCheck c2 = sph::check_bvh(sph::build_bvh_lbvh(b, leaf), b, leaf);
        const bool          ok = c.errors == 0 && c.hash == c2.hash && c.max_leaf <= leaf && c.slots == (int64_t)b.size() &&
                        (b.empty() ? c.nodes == 0 : c.nodes == 2 * c.leaves - 1);
        std::printf("%-16s lbvh leaf %d: nodes %lld leaves %lld depth %d max_leaf %d errors %lld kind %d %s\n", name.c_str(), leaf,
                    (long long)c.nodes, (long long)c.leaves, c.depth, c.max_leaf, (long long)c.errors, c.first_error_kind,
                    ok ? "ok" : "FAILED");
        failures += !ok;
    }
    {
        const sph::BvhCheck c = sph::check_bvh(sph::build_bvh_sah(b, 4), b, 4);
        std::printf("%-16s sah: nodes %lld depth %d errors %lld kind %d\n", name.c_str(), (long long)c.nodes, c.depth,
                    (long long)c.errors, c.first_error_kind);
        failures += c.errors != 0;
    }
    {
        const sph::BvhCheck c = sph::check_bvh(sph::build_bvh_reference(b), b, 0);
        std::printf("%-16s reference: nodes %lld depth %d errors %lld kind %d\n", name.c_str(), (long long)c.nodes, c.depth,
                    (long long)c.errors, c.first_error_kind);
        failures += c.errors != 0;
    }
}

int main()
{
    for (size_t n : { 0, 1, 2, 3, 4, 5, 8, 9, 63, 64, 65, 255, 256, 257, 1025 }) run("random" + std::to_string(n), random_set(n, 3u + (unsigned)n));
    run("identical37", std::vector<PrimBounds>(37, box(0.1f, 0.2f, 0.3f, 0.5f)));
    {
        std::vector<PrimBounds> v = random_set(64, 5);
        v.insert(v.end(), v.begin(), v.begin() + 32);
        run("half_dup", v);
    }
    {
        std::vector<PrimBounds> v = random_set(100, 6);
        for (auto& b : v) { b.lo[2] = -0.25f; b.hi[2] = 0.25f; }
        run("planar", v);
        for (auto& b : v) { b.lo[1] = -0.5f; b.hi[1] = 0.5f; }
        run("collinear", v);
    }
    {
        std::vector<PrimBounds> v; // the wedge strip's range of scales: most centroids in one cell
        for (int i = -80; i <= 135; ++i) {
            const float x = std::pow(1.9f, (float)i);
            v.push_back(PrimBounds{ { x, -0.5f * x, 0.0f }, { 1.25f * x, 0.5f * x, 0.0f } });
        }
        run("wedge", v);
    }
    {
        // an infinite bound gives a valid tree; a NaN bound (which sse_min / sse_max merges do not
        // carry, in any of the builders) must only leave the build and the checker in bounds
        std::vector<PrimBounds> v = random_set(50, 8), w = v;
        w[3].lo[0] = w[3].hi[0] = NAN;
        (void)sph::check_bvh(sph::build_bvh_lbvh(w, 4), w, 4);
        v[7].hi[1] = INFINITY;
        for (int leaf : { 1, 4 }) {
            const sph::Bvh t = sph::build_bvh_lbvh(v, leaf);
            const auto     c = sph::check_bvh(t, v, leaf);
            std::printf("nonfinite        lbvh leaf %d: nodes %lld depth %d errors %lld kind %d\n", leaf, (long long)c.nodes, c.depth,
                        (long long)c.errors, c.first_error_kind);
            failures += c.errors != 0;
        }
    }
    {
        // the checker itself: a broken tree must be reported
        std::vector<PrimBounds> v = random_set(40, 9);
        sph::Bvh                t = sph::build_bvh_lbvh(v, 2);
        sph::Bvh                a = t, b = t, c = t;
        a.nodes[0].hi[0] = a.nodes[0].lo[0]; // a box that is too small
        b.nodes[0].b = (uint32_t)b.nodes.size(); // a child out of range
        std::swap(c.prim_order[0], c.prim_order[1]);
        c.prim_order[1] = c.prim_order[0]; // not a permutation
        const bool seen = sph::check_bvh(a, v, 2).first_error_kind == sph::BVH_ERR_BOX &&
                          sph::check_bvh(b, v, 2).first_error_kind == sph::BVH_ERR_CHILD_RANGE &&
                          sph::check_bvh(c, v, 2).first_error_kind == sph::BVH_ERR_PRIM_ORDER && sph::check_bvh(t, v, 1).errors > 0;
        std::printf("checker reports broken trees: %s\n", seen ? "ok" : "FAILED");
        failures += !seen;
    }
    std::printf("%d failing\n", failures);
    return failures ? 1 : 0;
}
