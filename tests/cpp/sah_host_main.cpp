// sah_host_main.cpp -- the recursive SAH build against its level-wise restatement (sp_bvh.cpp
// build_bvh_sah, build_bvh_sah_levels) on seeded random and degenerate bound sets,
// as a stand-alone program so that it can run under -fsanitize=address,undefined
// (tests/test_device_sah_host.py compiles and runs it).  The two must agree on every node byte,
// the primitive order and the depth.  Prints a line per failing case and a summary; exit status 0
// only when none fails.
#include "../../simplepath_amd/csrc/host/sp_host.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

using sph::PrimBounds;

static PrimBounds box(float x, float y, float z, float r)
{
    return PrimBounds{ { x - r, y - r, z - r }, { x + r, y + r, z + r } };
}

static std::vector<PrimBounds> random_set(size_t n, unsigned seed, float scale = 1.0f)
{
    std::mt19937                          g(seed);
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    std::vector<PrimBounds>               v;
    v.reserve(n);
    for (size_t i = 0; i < n; ++i) v.push_back(box(scale * u(g), scale * u(g), scale * u(g), scale * (0.01f + 0.02f * std::fabs(u(g)))));
    return v;
}

static int failures = 0, cases = 0;

static void run(const std::string& name, const std::vector<PrimBounds>& b, int leaf_lo = 1, int leaf_hi = 4)
{
    for (int leaf = leaf_lo; leaf <= leaf_hi; ++leaf) {
        const sph::Bvh r = sph::build_bvh_sah(b, leaf), l = sph::build_bvh_sah_levels(b, leaf);
        const bool     nodes = r.nodes.size() == l.nodes.size() &&
                           (r.nodes.empty() || std::memcmp(r.nodes.data(), l.nodes.data(), r.nodes.size() * sizeof(sph::BvhNode)) == 0);
        const bool     ok    = nodes && r.prim_order == l.prim_order && r.max_depth == l.max_depth;
        const auto     c     = sph::check_bvh(l, b, leaf);
        ++cases;
        if (!ok || c.errors != 0) {
            std::printf("%-20s leaf %d: nodes %zu / %zu depth %d / %d nodes %s order %s errors %lld FAILED\n", name.c_str(), leaf,
                        r.nodes.size(), l.nodes.size(), r.max_depth, l.max_depth, nodes ? "equal" : "differ",
                        r.prim_order == l.prim_order ? "equal" : "differs", (long long)c.errors);
            ++failures;
        }
    }
}

int main()
{
    for (size_t n = 0; n <= 40; ++n) run("random" + std::to_string(n), random_set(n, 3u + (unsigned)n));
    {
        std::mt19937 g(99);
        for (int k = 0; k < 40; ++k) {
            const size_t n = 41 + g() % 4960; // up to 5000
            run("random" + std::to_string(n), random_set(n, 1000u + (unsigned)k), 1 + k % 4, 1 + k % 4);
        }
    }
    run("random5000", random_set(5000, 17));
    run("identical37", std::vector<PrimBounds>(37, box(0.1f, 0.2f, 0.3f, 0.5f)));
    run("identical1000", std::vector<PrimBounds>(1000, box(0.0f, 0.0f, 0.0f, 0.25f)));
    for (int k = 0; k < 6; ++k) { // duplicates: every box several times, far apart in the order
        std::vector<PrimBounds> v = random_set(40 + 37 * (size_t)k, 50u + (unsigned)k), w = v;
        for (int r = 0; r < 3; ++r) w.insert(w.end(), v.begin(), v.end());
        run("dup" + std::to_string(w.size()), w);
    }
    for (int k = 0; k < 6; ++k) { // zero-extent axes
        std::vector<PrimBounds> v = random_set(100 + 150 * (size_t)k, 60u + (unsigned)k);
        for (auto& b : v) { b.lo[2] = -0.25f; b.hi[2] = 0.25f; }
        run("planar" + std::to_string(v.size()), v);
        for (auto& b : v) { b.lo[1] = -0.5f; b.hi[1] = 0.5f; }
        run("collinear" + std::to_string(v.size()), v);
        for (auto& b : v) { b.lo[2] = b.hi[2] = 0.0f; }
        run("flat" + std::to_string(v.size()), v);
    }
    for (int k = 0; k < 8; ++k) { // +0 and -0 as box extremes, in both orders, and as centroids
        std::mt19937                          g(70u + (unsigned)k);
        std::uniform_real_distribution<float> u(0.0f, 1.0f);
        std::vector<PrimBounds>               v;
        const size_t                          n = 30 + 97 * (size_t)k;
        for (size_t i = 0; i < n; ++i) {
            const float z0 = (g() & 1u) ? 0.0f : -0.0f, z1 = (g() & 1u) ? 0.0f : -0.0f;
            PrimBounds  b{ { z0, -u(g), z1 }, { u(g), z1, z0 } };
            if (g() % 3u == 0u) b = PrimBounds{ { -u(g), z0, z0 }, { z1, u(g), z1 } };
            if (g() % 5u == 0u) b = PrimBounds{ { z0, z1, z0 }, { z1, z0, z1 } };
            v.push_back(b);
        }
        run("zeros" + std::to_string(n), v);
    }
    {
        std::vector<PrimBounds> v; // lattice: equal costs on two axes and at mirror bins
        for (int i = 0; i < 16; ++i)
            for (int j = 0; j < 16; ++j) v.push_back(box((float)i / 8.0f, (float)j / 8.0f, 0.0f, 1.0f / 64.0f));
        run("grid16", v);
    }
    {
        std::vector<PrimBounds> v; // a range of scales: most centroids in one bin
        for (int i = -80; i <= 135; ++i) {
            const float x = std::pow(1.9f, (float)i);
            v.push_back(PrimBounds{ { x, -0.5f * x, 0.0f }, { 1.25f * x, 0.5f * x, 0.0f } });
        }
        run("wedge", v);
    }
    for (int k = 0; k < 4; ++k) { // huge extents: areas and costs overflow to inf, centroid sums to +-inf
        std::vector<PrimBounds> v = random_set(200 + 300 * (size_t)k, 80u + (unsigned)k, 1.5e38f);
        run("huge" + std::to_string(v.size()), v);
        std::vector<PrimBounds> w = random_set(300, 90u + (unsigned)k, 1e19f);
        w.insert(w.end(), v.begin(), v.begin() + 50);
        run("huge_mixed" + std::to_string(k), w);
    }
    {
        std::vector<PrimBounds> v = random_set(3, 5, 0.05f), w = random_set(300, 6, 0.5f); // one child a leaf at once
        for (auto& b : v) { b.lo[0] -= 40.0f; b.hi[0] -= 40.0f; }
        v.insert(v.end(), w.begin(), w.end());
        run("two_clusters", v);
    }
    run("random200000", random_set(200000, 123), 4, 4);
    std::printf("%d cases\n%d failing\n", cases, failures);
    return failures ? 1 : 0;
}
