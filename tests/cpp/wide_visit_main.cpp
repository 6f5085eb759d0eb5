// wide_visit_main.cpp -- the one-exit visit of an 8-wide node (csrc/common/sp_wide_visit.h) against
// the branching form it replaced, restated below as the specification: wide_visit + slab_box as
// sp_path.hpp had them (eight slots, two `continue`s, three early returns and three swap-ifs per
// slot, std::max / std::min as compare-selects).  Every output word is compared -- inner, leaf,
// nearest and the bits of t_rest -- under both NAN_SAFE values.  A stand-alone program, so that it
// also runs under -fsanitize=address,undefined (tests/test_wide_visit_host.py compiles and runs it).
//
//   wide_visit_main                 the whole check; prints the pair counts, exit 0 when none differs
//   wide_visit_main dump N in out   N of the same pairs as rows for the device test
//                                   (tests/cpp/wide_visit_units.hip): in = 32 words per pair
//                                   (node 20, origin 3, inverse direction 3, tmin, tmax, filter, 3 of
//                                   padding), out = 8 words (the four results without and with NAN_SAFE)
//   wide_visit_main dumpw N in out  the same, but rows 64k .. 64k + 63 (one wave of the device test)
//                                   share row 64k's record and filter, each with a ray of its own:
//                                   the waves for which the device steps over slots nobody wants
#include "../../simplepath_amd/csrc/host/sp_host.hpp"
#include "../../simplepath_amd/csrc/common/sp_wide_visit.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <algorithm>
#include <string>
#include <thread>
#include <vector>

using sph::PrimBounds;

// ------------------------------------------------------------------ the specification
namespace spec {
static float std_max(float a, float b) { return (a < b) ? b : a; }
static float std_min(float a, float b) { return (b < a) ? b : a; }
static const float k_infinite = 3.40282346638528859812e+38f;

static bool slab_box(float lx, float ly, float lz, float hx, float hy, float hz, const float* o, const float* inv, float tmin,
                     float tmax, float& t0_out)
{
    float t0 = tmin, t1 = tmax;
    {
        float tn = (lx - o[0]) * inv[0], tf = (hx - o[0]) * inv[0];
        if (tn > tf) { const float s = tn; tn = tf; tf = s; }
        t0 = std_max(tn, t0);
        t1 = std_min(tf, t1);
        if (t0 > t1) return false;
    }
    {
        float tn = (ly - o[1]) * inv[1], tf = (hy - o[1]) * inv[1];
        if (tn > tf) { const float s = tn; tn = tf; tf = s; }
        t0 = std_max(tn, t0);
        t1 = std_min(tf, t1);
        if (t0 > t1) return false;
    }
    {
        float tn = (lz - o[2]) * inv[2], tf = (hz - o[2]) * inv[2];
        if (tn > tf) { const float s = tn; tn = tf; tf = s; }
        t0 = std_max(tn, t0);
        t1 = std_min(tf, t1);
        if (t0 > t1) return false;
    }
    t0_out = t0;
    return true;
}
static float ubyte(uint32_t w, int k) { return (float)((w >> (8 * (k & 3))) & 0xffu); }
static float u2f(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

static spw::Visit wide_visit(bool nan_safe, const uint32_t* w, const float* o, const float* inv, float tmin, float tmax,
                             uint32_t filter)
{
    const float    px = u2f(w[0]), py = u2f(w[1]), pz = u2f(w[2]);
    const float    sx = u2f((w[3] & 0xffu) << 23);
    const float    sy = u2f(((w[3] >> 8) & 0xffu) << 23);
    const float    sz = u2f(((w[3] >> 16) & 0xffu) << 23);
    const uint32_t imask = w[3] >> 24;
    spw::Visit     r;
    r.inner = 0; r.leaf = 0; r.nearest = -1; r.t_rest = k_infinite;
    float best = k_infinite;
    for (int k = 0; k < 8; ++k) {
        const uint32_t meta  = ((k < 4 ? w[6] : w[7]) >> (8 * (k & 3))) & 0xffu;
        const bool     inner = (imask >> k) & 1u;
        if (!inner && meta == 0u) continue;
        if (!((filter >> k) & 1u)) continue;
        const int   h  = k >> 2;
        const float lx = std::fma(ubyte(w[8 + h], k), sx, px);
        const float ly = std::fma(ubyte(w[10 + h], k), sy, py);
        const float lz = std::fma(ubyte(w[12 + h], k), sz, pz);
        const float hx = std::fma(ubyte(w[14 + h], k), sx, px);
        const float hy = std::fma(ubyte(w[16 + h], k), sy, py);
        const float hz = std::fma(ubyte(w[18 + h], k), sz, pz);
        float       t0;
        if (!slab_box(lx, ly, lz, hx, hy, hz, o, inv, tmin, tmax, t0)) continue;
        if (nan_safe) t0 = (t0 == t0) ? t0 : -k_infinite;
        if (inner) {
            r.inner |= 1u << k;
            if (t0 < best) { r.t_rest = best; best = t0; r.nearest = k; }
            else r.t_rest = std_min(r.t_rest, t0);
        } else {
            r.leaf |= 1u << k;
        }
    }
    if (nan_safe)
        if (r.inner && r.nearest < 0) r.nearest = __builtin_ffs((int)r.inner) - 1;
    return r;
}
} // namespace spec

// ------------------------------------------------------------------ inputs
struct Rng { // splitmix64
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
    uint32_t u32() { return (uint32_t)(next() >> 32); }
    uint32_t below(uint32_t n) { return (uint32_t)((next() >> 33) % n); }
    float    unit() { return (float)(next() >> 40) * (1.0f / 16777216.0f); } // [0, 1)
    float    sym() { return 2.0f * unit() - 1.0f; }
};

struct Pair {
    uint32_t w[20];
    float    o[3], inv[3], tmin, tmax;
    uint32_t filter;
};

static const float INF = std::numeric_limits<float>::infinity();
static const float QNAN = std::numeric_limits<float>::quiet_NaN();
// the components the issue names: signed zeros, denormals, the smallest denormal, infinities, NaN
static const float SPECIAL[] = { 0.0f, -0.0f, 1e-40f, -1e-40f, 1.4e-45f, -1.4e-45f, INF, -INF, QNAN, 1.0f, -1.0f, 3.0e38f, 1e-30f };
static const int   N_SPECIAL = (int)(sizeof(SPECIAL) / sizeof(SPECIAL[0]));

static PrimBounds box(float x, float y, float z, float r) { return PrimBounds{ { x - r, y - r, z - r }, { x + r, y + r, z + r } }; }

// the kinds of primitive sets the ray-query tests build: scattered, planar, duplicated, zero extent
static std::vector<std::vector<PrimBounds>> prim_sets()
{
    std::vector<std::vector<PrimBounds>> sets;
    Rng g{ 11 };
    for (size_t n : { 13u, 64u, 300u, 1025u }) {
        std::vector<PrimBounds> v;
        for (size_t i = 0; i < n; ++i) v.push_back(box(g.sym(), g.sym(), g.sym(), 0.01f + 0.03f * g.unit()));
        sets.push_back(v);
    }
    {
        std::vector<PrimBounds> v = sets[1];
        for (auto& b : v) { b.lo[2] = -0.25f; b.hi[2] = -0.25f; } // planar, zero extent on z
        sets.push_back(v);
    }
    {
        std::vector<PrimBounds> v = sets[1];
        v.insert(v.end(), v.begin(), v.begin() + 40); // duplicated boxes: equal entry distances
        sets.push_back(v);
    }
    sets.push_back(std::vector<PrimBounds>(20, box(0.25f, -0.5f, 0.125f, 0.0f))); // points
    return sets;
}

static std::vector<uint32_t> real_nodes()
{
    std::vector<uint32_t> words;
    for (const auto& b : prim_sets())
        for (int leaf : { 1, 4 }) {
            const sph::WideBvh a = sph::build_wide(sph::build_bvh_sah(b, leaf));
            words.insert(words.end(), a.words.begin(), a.words.end());
            const sph::WideBvh l = sph::build_wide(sph::build_bvh_lbvh(b, leaf));
            words.insert(words.end(), l.words.begin(), l.words.end());
        }
    return words;
}

static float decoded(const uint32_t* w, int row, int k, int axis)
{
    const float p = spec::u2f(w[axis]), s = spec::u2f(((w[3] >> (8 * axis)) & 0xffu) << 23);
    return std::fma(spec::ubyte(w[8 + 2 * row + (k >> 2)], k), s, p);
}

static void set_inv(Pair& p, const float* d)
{
    for (int a = 0; a < 3; ++a) p.inv[a] = 1.0f / d[a];
}

// d: from the origin to a point of the node's quantisation grid, any length
static void aim(const Pair& p, Rng& g, float* d)
{
    const float len = 0.25f + 2.0f * g.unit();
    for (int a = 0; a < 3; ++a) {
        const float s = spec::u2f(((p.w[3] >> (8 * a)) & 0xffu) << 23);
        d[a] = (std::fma(255.0f * g.unit(), s, spec::u2f(p.w[a])) - p.o[a]) * len;
    }
}

// (a) a real node with a camera-like, a random or an in-box-plane ray
static Pair real_pair(const std::vector<uint32_t>& nodes, Rng& g)
{
    Pair p;
    const size_t n = nodes.size() / 20;
    std::memcpy(p.w, &nodes[20 * g.below((uint32_t)n)], 80);
    float d[3];
    const uint32_t kind = g.below(3);
    if (kind == 0) { // camera-like: one origin, directions through an image plane or at the node
        p.o[0] = 0.1f; p.o[1] = 0.2f; p.o[2] = 3.2f;
        d[0] = 0.8f * g.sym(); d[1] = 0.6f * g.sym(); d[2] = -1.0f;
        if (g.below(2)) aim(p, g, d);
    } else if (kind == 1) { // random, mostly through the node's own extent
        for (int a = 0; a < 3; ++a) { p.o[a] = 2.0f * g.sym(); d[a] = g.sym(); }
        if (g.below(4)) aim(p, g, d);
    } else { // the origin exactly in a decoded plane of a slot, the direction component there tiny or zero
        for (int a = 0; a < 3; ++a) { p.o[a] = 1.5f * g.sym(); d[a] = g.sym(); }
        const int a = (int)g.below(3), k = (int)g.below(8);
        p.o[a] = decoded(p.w, (g.below(2) ? 3 : 0) + a, k, a);
        d[a]   = SPECIAL[g.below(6)];
    }
    set_inv(p, d);
    p.tmin   = g.below(4) ? 0.001f : 0.0f;
    const uint32_t tm = g.below(4);
    p.tmax   = tm == 0 ? INF : tm == 1 ? spec::k_infinite : 4.0f * g.unit();
    p.filter = g.below(4) ? 0xffu : g.u32();
    return p;
}

// (b) a synthetic record with a ray of special components
static Pair synthetic_pair(Rng& g, uint32_t index)
{
    Pair p;
    for (int i = 0; i < 20; ++i) p.w[i] = g.u32();
    // origin and scale: mostly moderate, sometimes any bit pattern (scale bytes 0 and 255 included)
    if (g.below(4)) {
        for (int a = 0; a < 3; ++a) p.w[a] = spm::f2u(g.sym());
        const uint32_t e = 110u + g.below(20);
        p.w[3] = (p.w[3] & 0xff000000u) | e | (110u + g.below(20)) << 8 | (110u + g.below(20)) << 16;
    }
    // every empty / leaf / inner slot pattern: slot states from the pair's index in base 3
    uint32_t imask = 0, meta[2] = { 0, 0 }, x = index;
    for (int k = 0; k < 8; ++k, x /= 3) {
        const uint32_t state = x % 3;
        if (state == 1) imask |= 1u << k;
        if (state == 2 || (state == 1 && g.below(2))) meta[k >> 2] |= (1u + g.below(255)) << (8 * (k & 3));
    }
    p.w[3] = (p.w[3] & 0x00ffffffu) | imask << 24;
    p.w[6] = meta[0];
    p.w[7] = meta[1];
    const uint32_t shape = g.below(4);
    if (shape == 0) { // duplicated child boxes: ties
        const uint32_t src = g.below(8);
        for (int k = 0; k < 8; ++k)
            if (g.below(2))
                for (int r = 0; r < 6; ++r) {
                    const uint32_t b = (p.w[8 + 2 * r + (src >> 2)] >> (8 * (src & 3))) & 0xffu;
                    uint32_t&      t = p.w[8 + 2 * r + (k >> 2)];
                    t = (t & ~(0xffu << (8 * (k & 3)))) | b << (8 * (k & 3));
                }
    } else if (shape == 1) { // zero-extent boxes: hi = lo
        for (int r = 0; r < 3; ++r) { p.w[14 + 2 * r] = p.w[8 + 2 * r]; p.w[15 + 2 * r] = p.w[9 + 2 * r]; }
    }
    if (g.below(4)) // mostly boxes with lo <= hi: the bytes of the three upper rows raised to the lower rows'
        for (int r = 0; r < 3; ++r)
            for (int h = 0; h < 2; ++h)
                for (int b = 0; b < 4; ++b) {
                    const uint32_t lo = (p.w[8 + 2 * r + h] >> (8 * b)) & 0xffu, hi = (p.w[14 + 2 * r + h] >> (8 * b)) & 0xffu;
                    if (hi < lo) p.w[14 + 2 * r + h] = (p.w[14 + 2 * r + h] & ~(0xffu << (8 * b))) | lo << (8 * b);
                }
    float d[3];
    for (int a = 0; a < 3; ++a) {
        p.o[a] = g.below(3) ? g.sym() : SPECIAL[g.below(N_SPECIAL)];
        d[a]   = g.below(2) ? g.sym() : SPECIAL[g.below(N_SPECIAL)];
    }
    if (g.below(2)) { // through the record's own extent, then one special component
        for (int a = 0; a < 3; ++a) p.o[a] = 2.0f * g.sym();
        aim(p, g, d);
        if (g.below(2)) d[g.below(3)] = SPECIAL[g.below(N_SPECIAL)];
    }
    if (g.below(3) == 0) { // an origin exactly in a decoded plane
        const int a = (int)g.below(3);
        p.o[a] = decoded(p.w, (g.below(2) ? 3 : 0) + a, (int)g.below(8), a);
    }
    set_inv(p, d);
    if (g.below(8) == 0) p.inv[g.below(3)] = SPECIAL[g.below(N_SPECIAL)]; // an inverse no direction gives, NaN included
    const uint32_t t0 = g.below(6), t1 = g.below(6);
    p.tmin   = t0 == 0 ? 0.0f : t0 == 1 ? -0.0f : t0 == 2 ? SPECIAL[g.below(N_SPECIAL)] : 0.001f;
    p.tmax   = t1 == 0 ? INF : t1 == 1 ? spec::k_infinite : t1 == 2 ? SPECIAL[g.below(N_SPECIAL)] : 3.0f * g.unit();
    p.filter = g.below(3) ? 0xffu : g.u32();
    return p;
}

static Pair make_pair_at(const std::vector<uint32_t>& nodes, Rng& g, uint64_t i)
{
    return (i & 1) ? synthetic_pair(g, (uint32_t)(i >> 1)) : real_pair(nodes, g);
}

struct Count {
    uint64_t bad = 0, with_inner = 0, with_leaf = 0, nan_rest = 0, ranked_rest = 0, differ_ns = 0, first = 0;
    Pair     first_pair;
};

static void results(const Pair& p, bool use_spec, uint32_t* out)
{
    for (int ns = 0; ns < 2; ++ns) {
        spw::Visit v;
        if (use_spec) v = spec::wide_visit(ns != 0, p.w, p.o, p.inv, p.tmin, p.tmax, p.filter);
        else if (ns) v = spw::visit<true>(p.w, p.o[0], p.o[1], p.o[2], p.inv[0], p.inv[1], p.inv[2], p.tmin, p.tmax, p.filter);
        else v = spw::visit<false>(p.w, p.o[0], p.o[1], p.o[2], p.inv[0], p.inv[1], p.inv[2], p.tmin, p.tmax, p.filter);
        out[4 * ns + 0] = v.inner;
        out[4 * ns + 1] = v.leaf;
        out[4 * ns + 2] = (uint32_t)v.nearest;
        out[4 * ns + 3] = spm::f2u(v.t_rest);
    }
}

int main(int argc, char** argv)
{
    const std::vector<uint32_t> nodes = real_nodes();
    if (argc == 5 && (std::string(argv[1]) == "dump" || std::string(argv[1]) == "dumpw")) {
        const bool shared = std::string(argv[1]) == "dumpw";
        const long n = std::atol(argv[2]);
        FILE *     fi = std::fopen(argv[3], "wb"), *fo = std::fopen(argv[4], "wb");
        if (n <= 0 || !fi || !fo) return 2;
        Rng  g{ 2024 }; // block 0 of the check, continued
        Pair leader = {};
        for (long i = 0; i < n; ++i) {
            Pair p = make_pair_at(nodes, g, (uint64_t)i);
            if (shared) { // the leader's record and filter, a ray of the lane's own near the leader's
                if (i % 64 == 0) leader = p;
                else {
                    p = leader;
                    for (int a = 0; a < 3; ++a) { p.o[a] += 0.05f * g.sym(); p.inv[a] *= 1.0f + 0.2f * g.sym(); }
                    if (i % 8 == 3) p.tmax = INF;
                    if (i % 8 == 5) { // 0 * inf in a slab of the shared record: a NaN entry distance
                        const int a = (int)g.below(3);
                        p.o[a]   = decoded(p.w, a, (int)g.below(8), a);
                        p.inv[a] = g.below(2) ? INF : -INF;
                    }
                }
            }
            uint32_t row[32] = { 0 }, out[8];
            std::memcpy(row, p.w, 80);
            std::memcpy(row + 20, p.o, 12);
            std::memcpy(row + 23, p.inv, 12);
            std::memcpy(row + 26, &p.tmin, 4);
            std::memcpy(row + 27, &p.tmax, 4);
            row[28] = p.filter;
            results(p, true, out); // the specification's words
            if (std::fwrite(row, 4, 32, fi) != 32 || std::fwrite(out, 4, 8, fo) != 8) return 2;
        }
        std::fclose(fi);
        std::fclose(fo);
        std::printf("dumped %ld pairs\n", n);
        return 0;
    }
    const uint64_t total = argc == 2 ? (uint64_t)std::atoll(argv[1]) : 12000000ull;
    // the byte mask on its own, every byte pattern class
    uint64_t bad_mask = 0;
    for (uint32_t i = 0; i < (1u << 16); ++i) {
        uint32_t w = 0, expect = 0;
        for (int j = 0; j < 4; ++j) {
            const uint32_t nib = (i >> (4 * j)) & 0xfu, b = nib == 0 ? 0u : nib == 15 ? 0xffu : 1u << (nib % 8);
            w |= b << (8 * j);
            expect |= (b != 0u ? 1u : 0u) << j;
        }
        bad_mask += spw::nonzero_bytes(w) != expect;
    }
    std::printf("nonzero_bytes: %s\n", bad_mask ? "FAILED" : "ok");
    // blocks of pairs, each from its own generator, dealt to a few threads
    const uint64_t     BLOCK = 1u << 14, blocks = (total + BLOCK - 1) / BLOCK;
    const unsigned     nt = std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    std::vector<Count> counts(nt);
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < nt; ++t)
        pool.emplace_back([&, t] {
            Count& c = counts[t];
            for (uint64_t blk = t; blk < blocks; blk += nt) {
                Rng            g{ 2024 + blk };
                const uint64_t end = std::min(total, (blk + 1) * BLOCK);
                for (uint64_t i = blk * BLOCK; i < end; ++i) {
                    const Pair p = make_pair_at(nodes, g, i);
                    uint32_t   want[8], got[8];
                    results(p, true, want);
                    results(p, false, got);
                    c.with_inner += want[0] != 0;
                    c.with_leaf += want[1] != 0;
                    c.nan_rest += (want[3] & 0x7fffffffu) > 0x7f800000u;
                    c.differ_ns += std::memcmp(want, want + 4, 16) != 0;
                    c.ranked_rest += want[0] != 0 && (want[0] & (want[0] - 1)) && want[3] != spm::f2u(spec::k_infinite);
                    if (std::memcmp(want, got, 32) != 0) {
                        if (c.bad == 0) { c.first = i; c.first_pair = p; }
                        ++c.bad;
                    }
                }
            }
        });
    for (auto& th : pool) th.join();
    uint64_t bad = 0, with_inner = 0, with_leaf = 0, nan_rest = 0, two_equal = 0, differ_ns = 0;
    for (const Count& c : counts) {
        bad += c.bad; with_inner += c.with_inner; with_leaf += c.with_leaf; nan_rest += c.nan_rest; two_equal += c.ranked_rest;
        differ_ns += c.differ_ns;
        if (c.bad) {
            const Pair& p = c.first_pair;
            uint32_t    want[8], got[8];
            results(p, true, want);
            results(p, false, got);
            std::printf("pair %llu differs:\n  want", (unsigned long long)c.first);
            for (int j = 0; j < 8; ++j) std::printf(" %08x", want[j]);
            std::printf("\n  got ");
            for (int j = 0; j < 8; ++j) std::printf(" %08x", got[j]);
            std::printf("\n  node");
            for (int j = 0; j < 20; ++j) std::printf(" %08x", p.w[j]);
            std::printf("\n  o %a %a %a inv %a %a %a tmin %a tmax %a filter %08x\n", p.o[0], p.o[1], p.o[2], p.inv[0], p.inv[1],
                        p.inv[2], p.tmin, p.tmax, p.filter);
        }
    }
    std::printf("%llu pairs (%zu real nodes): %llu with inner hits, %llu with leaf hits, %llu with a ranked rest, "
                "%llu where NAN_SAFE changes a word, %llu with a NaN t_rest\n",
                (unsigned long long)total, nodes.size() / 20, (unsigned long long)with_inner, (unsigned long long)with_leaf,
                (unsigned long long)two_equal, (unsigned long long)differ_ns, (unsigned long long)nan_rest);
    std::printf("%llu failing\n", (unsigned long long)(bad + bad_mask));
    return (bad || bad_mask) ? 1 : 0;
}
