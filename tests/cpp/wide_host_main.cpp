// wide_host_main.cpp -- the 8-wide collapse (sp_bvh.cpp build_wide), its level-wise restatement
// (build_wide_levels, what the device finish runs) and the wide-tree checker on constructed bounds,
// as a stand-alone program so that it can run under -fsanitize=address,undefined
// (tests/test_device_finish_host.py compiles and runs it).  Prints one line per case and a summary;
// exit status 0 only when both collapses agree word for word, every tree passes the checker, and
// the checker names each planted damage.
#include "../../simplepath_amd/csrc/host/sp_host.hpp"
#include "../../simplepath_amd/csrc/common/sp_wide.h"

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

static std::vector<PrimBounds> random_set(size_t n, unsigned seed)
{
    std::mt19937                          g(seed);
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    std::vector<PrimBounds>               v;
    for (size_t i = 0; i < n; ++i) v.push_back(box(u(g), u(g), u(g), 0.01f + 0.02f * std::fabs(u(g))));
    return v;
}

static int failures = 0;

static void run_tree(const std::string& name, const char* builder, int leaf, const sph::Bvh& t, const std::vector<PrimBounds>& b)
{
    const sph::WideBvh   a = sph::build_wide(t), l = sph::build_wide_levels(t);
    const sph::WideCheck c = sph::check_wide(l, t.prim_order, b);
    const bool           same = a.words == l.words && a.slot_of == l.slot_of && a.depth == l.depth;
    const bool           ok   = same && c.errors == 0 && sph::check_wide(a, t.prim_order, b).errors == 0 &&
                    c.slots == (int64_t)b.size() && (b.empty() ? c.records == 0 : c.records >= 1);
    std::printf("%-16s %-6s leaf %d: records %lld holes %lld slots %lld depth %d errors %lld kind %d %s\n", name.c_str(), builder,
                leaf, (long long)c.records, (long long)c.holes, (long long)c.slots, c.depth, (long long)c.errors, c.first_error_kind,
                ok ? "ok" : (same ? "FAILED" : "FAILED (the two collapses differ)"));
    failures += !ok;
}

static void run(const std::string& name, const std::vector<PrimBounds>& b)
{
    for (int leaf : { 1, 2, 4 }) {
        run_tree(name, "lbvh", leaf, sph::build_bvh_lbvh(b, leaf), b);
        run_tree(name, "sah", leaf, sph::build_bvh_sah(b, leaf), b);
    }
}

static void planted(const char* what, const sph::WideBvh& w, const sph::Bvh& t, const std::vector<PrimBounds>& b, int expect)
{
    const sph::WideCheck c  = sph::check_wide(w, t.prim_order, b);
    const bool           ok = c.errors > 0 && c.first_error_kind == expect;
    std::printf("planted %s: errors %lld kind %d (expected %d) node %lld %s\n", what, (long long)c.errors, c.first_error_kind, expect,
                (long long)c.first_error_node, ok ? "ok" : "FAILED");
    failures += !ok;
}

int main()
{
    // the exponent of sp_wide.h against frexpf, over every exponent and the denormals
    {
        int bad = 0;
        for (uint32_t e = 0; e < 255; ++e)
            for (uint32_t m : { 0u, 1u, 0x400000u, 0x7fffffu, 0x000100u }) {
                const uint32_t u = e << 23 | m;
                float          x;
                std::memcpy(&x, &u, 4);
                int e2 = 0;
                std::frexp(x, &e2);
                bad += spw::frexp_exp(x) != e2;
                if (e >= 1 && e <= 254 && m == 0) bad += spw::pow2((int)e - 127) != std::ldexp(1.0f, (int)e - 127);
            }
        std::printf("frexp / ldexp restatements: %s\n", bad ? "FAILED" : "ok");
        failures += bad != 0;
    }
    for (size_t n : { 0, 1, 2, 3, 4, 5, 8, 9, 63, 64, 65, 255, 256, 257, 1025 }) run("random" + std::to_string(n), random_set(n, 3u + (unsigned)n));
    run("identical37", std::vector<PrimBounds>(37, box(0.1f, 0.2f, 0.3f, 0.5f)));
    run("points", std::vector<PrimBounds>(20, box(0.25f, -0.5f, 0.125f, 0.0f))); // zero extent: k = -126
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
        std::vector<PrimBounds> v; // the wedge strip's range of scales: steps from 2^-126 upwards
        for (int i = -80; i <= 135; ++i) {
            const float x = std::pow(1.9f, (float)i);
            v.push_back(PrimBounds{ { x, -0.5f * x, 0.0f }, { 1.25f * x, 0.5f * x, 0.0f } });
        }
        run("wedge", v);
    }
    {
        // empty boxes (lo > hi: NaN scores in the slot assignment) must only stay in bounds
        std::vector<PrimBounds> v = random_set(50, 8);
        for (int i : { 3, 4, 17 })
            for (int a = 0; a < 3; ++a) { v[(size_t)i].lo[a] = INFINITY; v[(size_t)i].hi[a] = -INFINITY; }
        for (int leaf : { 1, 4 }) {
            const sph::Bvh     t = sph::build_bvh_lbvh(v, leaf);
            const sph::WideBvh a = sph::build_wide(t), l = sph::build_wide_levels(t);
            const bool         same = a.words == l.words && a.slot_of == l.slot_of && a.depth == l.depth;
            std::printf("empty boxes      leaf %d: %s\n", leaf, same ? "ok" : "FAILED");
            failures += !same;
            (void)sph::check_wide(l, t.prim_order, v);
        }
    }
    {
        // the checker itself: one thing damaged at a time on a copy of a valid tree
        std::vector<PrimBounds> v = random_set(300, 9);
        const sph::Bvh          t = sph::build_bvh_sah(v, 2);
        const sph::WideBvh      w = sph::build_wide(t);
        const sph::WideCheck    c = sph::check_wide(w, t.prim_order, v);
        if (c.errors != 0 || c.holes < 1 || c.records < 10) {
            std::printf("planted: the base tree is not fit for the test (errors %lld holes %lld)\n", (long long)c.errors, (long long)c.holes);
            ++failures;
        }
        const uint32_t root_imask = w.words[3] >> 24;
        int            inner = -1; // an inner slot of the root
        for (int s = 0; s < 8; ++s)
            if ((root_imask >> s) & 1u) inner = s;
        {
            sph::WideBvh d = w;
            d.words[4]     = (uint32_t)(d.words.size() / 20); // child_base past the last record
            planted("child_base", d, t, v, sph::WIDE_ERR_CHILD_RANGE);
        }
        {
            // a count of 0 on an occupied leaf slot: one with an offset, so that the byte stays non-zero
            sph::WideBvh d = w;
            bool         done = false;
            for (size_t rec = 0; rec < d.words.size() / 20 && !done; ++rec)
                for (int s = 0; s < 8 && !done; ++s) {
                    uint32_t& m = d.words[20 * rec + 6 + (size_t)s / 4];
                    if (((m >> (8 * (s % 4))) & 0x1fu) == 0u) continue;
                    m &= ~(0xe0u << (8 * (s % 4)));
                    done = true;
                }
            planted("meta count", d, t, v, sph::WIDE_ERR_META);
        }
        {
            // the upper bound of an inner child of the root moved inward by one step on x
            sph::WideBvh d = w;
            const int    s = inner >= 0 ? inner : 0;
            uint32_t&    q = d.words[8 + 2 * 3 + (size_t)s / 4];
            const uint32_t byte = (q >> (8 * (s % 4))) & 0xffu;
            q = (q & ~(0xffu << (8 * (s % 4)))) | ((byte - 1u) & 0xffu) << (8 * (s % 4));
            planted("quantised byte", d, t, v, sph::WIDE_ERR_BOX);
        }
        {
            sph::WideBvh   d = w;
            std::vector<uint8_t> reached(d.words.size() / 20, 0);
            reached[0] = 1;
            for (size_t r = 0; r < reached.size(); ++r) // records come after their parents
                for (int s = 0; s < 8; ++s)
                    if (reached[r] && ((d.words[20 * r + 3] >> (24 + s)) & 1u)) reached[d.words[20 * r + 4] + (size_t)s] = 1;
            size_t hole = 0;
            while (hole < reached.size() && reached[hole]) ++hole;
            if (hole < reached.size()) d.words[20 * hole + 9] = 7u;
            planted("hole", d, t, v, sph::WIDE_ERR_HOLE);
        }
    }
    std::printf("%d failing\n", failures);
    return failures ? 1 : 0;
}
