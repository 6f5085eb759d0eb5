// wide_visit_plain_main.cpp -- spw::visit_plain (csrc/common/sp_wide_visit.h: near / far chosen on the
// packed words, min / max instructions, one interval test per slot) against spw::visit<false>, under
// visit_plain's contract: inner, leaf and nearest exactly, t_rest equal as a float value.  Inside the
// contract nothing may differ; outside it (rays that spw::plain_ray rejects) the program counts the
// pairs that do differ, which is why the walks ask the predicate first.  A stand-alone program, so
// that it also runs under -fsanitize=address,undefined (tests/test_wide_visit_plain_host.py).
//
//   wide_visit_plain_main [N]            the whole check over N pairs (default 1.6e7, of which over 1e7 fall inside the contract); prints the
//                                        class counts, exit 0 when no pair inside the contract differs
//   wide_visit_plain_main dump N in out  N of the pairs inside the contract as rows for the device
//                                        test (tests/cpp/wide_visit_plain_units.hip): in = 32 words per
//                                        pair (node 20, origin 3, inverse direction 3, tmin, tmax,
//                                        filter, 3 of padding), out = visit<false>'s four words
//   wide_visit_plain_main walk out       one small tree and 256 rays for the device walks: words
//                                        {records, slots, depth, rays}, the node words, 12 floats per
//                                        wide slot (p0 | code, p1, p2), 8 floats per ray (o, tmin, d, tmax)
#include "../../simplepath_amd/csrc/host/sp_host.hpp"
#include "../../simplepath_amd/csrc/common/sp_wide_visit.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <thread>
#include <vector>

using sph::PrimBounds;

namespace {

const float INF  = std::numeric_limits<float>::infinity();
const float QNAN = std::numeric_limits<float>::quiet_NaN();

struct Rng { // splitmix64
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
    uint32_t u32() { return (uint32_t)(next() >> 32); }
    uint32_t below(uint32_t n) { return (uint32_t)((next() >> 33) % n); }
    float    unit() { return (float)(next() >> 40) * (1.0f / 16777216.0f); } // [0, 1)
    float    sym() { return 2.0f * unit() - 1.0f; }
    float    nz() { const float v = sym(); return v == 0.0f ? 0.5f : v; } // (-1, 1) without zero
};

struct Pair {
    uint32_t w[20];
    float    o[3], inv[3], tmin, tmax;
    uint32_t filter;
};

float    u2f(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
uint32_t f2u(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
uint32_t qbyte(const uint32_t* w, int row, int k) { return (w[8 + 2 * row + (k >> 2)] >> (8 * (k & 3))) & 0xffu; } // rows 0-2 lo xyz, 3-5 hi xyz
float    scale(const uint32_t* w, int axis) { return u2f(((w[3] >> (8 * axis)) & 0xffu) << 23); }
float    decoded(const uint32_t* w, int row, int k) { return std::fma((float)qbyte(w, row, k), scale(w, row % 3), u2f(w[row % 3])); }
uint32_t valid_slots(const uint32_t* w, uint32_t filter)
{
    return ((w[3] >> 24) | spw::nonzero_bytes(w[6]) | spw::nonzero_bytes(w[7]) << 4) & filter & 0xffu;
}

PrimBounds box(float x, float y, float z, float r) { return PrimBounds{ { x - r, y - r, z - r }, { x + r, y + r, z + r } }; }

// scattered, planar, duplicated and point sets, through both host builders at leaf sizes 1 and 4
std::vector<uint32_t> real_nodes()
{
    std::vector<std::vector<PrimBounds>> sets;
    Rng g{ 29 };
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
    std::vector<uint32_t> words;
    for (const auto& b : sets)
        for (int leaf : { 1, 4 }) {
            const sph::WideBvh a = sph::build_wide(sph::build_bvh_sah(b, leaf));
            words.insert(words.end(), a.words.begin(), a.words.end());
            const sph::WideBvh l = sph::build_wide(sph::build_bvh_lbvh(b, leaf));
            words.insert(words.end(), l.words.begin(), l.words.end());
        }
    return words;
}

// the node side of the contract: finite origin, scale bytes <= 254, qlo <= qhi on occupied-and-wanted slots
bool node_in_contract(const Pair& p)
{
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(u2f(p.w[a]))) return false;
        if (((p.w[3] >> (8 * a)) & 0xffu) > 254u) return false;
    }
    const uint32_t valid = valid_slots(p.w, p.filter);
    for (int k = 0; k < 8; ++k)
        if ((valid >> k) & 1u)
            for (int a = 0; a < 3; ++a)
                if (qbyte(p.w, a, k) > qbyte(p.w, 3 + a, k)) return false;
    return true;
}

bool ray_plain(const Pair& p) { return spw::plain_ray(p.o[0], p.o[1], p.o[2], p.inv[0], p.inv[1], p.inv[2], p.tmin, p.tmax); }

// d: from the origin to a point of the node's quantisation grid, any length
void aim(const Pair& p, Rng& g, float* d)
{
    const float len = 0.25f + 2.0f * g.unit();
    for (int a = 0; a < 3; ++a) {
        d[a] = (std::fma(255.0f * g.unit(), scale(p.w, a), u2f(p.w[a])) - p.o[a]) * len;
        if (d[a] == 0.0f) d[a] = 0.25f;
    }
}

// one component outside the ray conditions: an inverse of +-inf (d = +-0 or a small denormal) or 0
// (d infinite), an infinite origin, a NaN tmin or tmax; the origin put in a box plane first where
// that is what makes a 0 * inf
void spoil(Pair& p, Rng& g)
{
    const int a = (int)g.below(3);
    switch (g.below(6)) {
    case 0: case 1:
        if (g.below(2)) p.o[a] = decoded(p.w, (g.below(2) ? 3 : 0) + a, (int)g.below(8));
        p.inv[a] = g.below(2) ? INF : -INF;
        break;
    case 2: p.inv[a] = g.below(2) ? 0.0f : -0.0f; break;
    case 3: p.o[a] = g.below(2) ? INF : -INF; break;
    case 4: p.tmin = QNAN; break;
    default: p.tmax = QNAN; break;
    }
}

void finish_ray(Pair& p, Rng& g, const float* d)
{
    for (int a = 0; a < 3; ++a) p.inv[a] = 1.0f / d[a];
    const uint32_t t0 = g.below(4), t1 = g.below(4);
    p.tmin = t0 == 0 ? 0.0f : t0 == 1 ? -0.0f : 0.001f;
    p.tmax = t1 == 0 ? INF : t1 == 1 ? 3.40282346638528859812e+38f : 4.0f * g.unit();
    if (g.below(4) == 0) spoil(p, g);
}

// a ray for the node in p.w: camera-like, random, axis-heavy (huge and tiny components: products that
// overflow), or starting exactly in a decoded plane of a slot with a plain direction
void make_ray(Pair& p, Rng& g)
{
    float d[3];
    switch (g.below(4)) {
    case 0: // camera-like: one origin, directions through an image plane or at the node
        p.o[0] = 0.1f; p.o[1] = 0.2f; p.o[2] = 3.2f;
        d[0] = 0.8f * g.nz(); d[1] = 0.6f * g.nz(); d[2] = -1.0f;
        if (g.below(2)) aim(p, g, d);
        break;
    case 1: // random, mostly through the node's own extent
        for (int a = 0; a < 3; ++a) { p.o[a] = 2.0f * g.sym(); d[a] = g.nz(); }
        if (g.below(4)) aim(p, g, d);
        break;
    case 2: // components of very different size: 1e-38 .. 1e30 directions, origins far off
        for (int a = 0; a < 3; ++a) {
            const uint32_t s = g.below(5);
            d[a]   = g.nz() * (s == 0 ? 1e30f : s == 1 ? 1e-30f : s == 2 ? 2.4e-38f : 1.0f);
            if (std::fabs(d[a]) < 1.2e-38f) d[a] = std::copysign(1.2e-38f, d[a]); // 1 / d stays finite
            p.o[a] = g.sym() * (g.below(3) ? 2.0f : 1e4f);
        }
        break;
    default: // the origin exactly in decoded planes of a slot (one, two or three axes), a plain direction
        for (int a = 0; a < 3; ++a) { p.o[a] = 1.5f * g.sym(); d[a] = g.nz(); }
        {
            const int k = (int)g.below(8), n = 1 + (int)g.below(3), a0 = (int)g.below(3);
            for (int j = 0; j < n; ++j) {
                const int a = (a0 + j) % 3;
                p.o[a] = decoded(p.w, (g.below(2) ? 3 : 0) + a, k);
            }
            if (g.below(2)) aim(p, g, d);
        }
        break;
    }
    finish_ray(p, g, d);
}

Pair real_pair(const std::vector<uint32_t>& nodes, Rng& g)
{
    Pair p;
    std::memcpy(p.w, &nodes[20 * (size_t)g.below((uint32_t)(nodes.size() / 20))], 80);
    make_ray(p, g);
    p.filter = g.below(4) ? 0xffu : g.u32();
    return p;
}

// a synthetic record: random bytes with qlo <= qhi, every empty / leaf / inner slot pattern (the slot
// states are the pair's index in base 3), duplicated and zero-extent boxes; one in 16 breaks the
// node side of the contract on purpose (a lower byte above its upper byte, a scale byte of 255)
Pair synthetic_pair(Rng& g, uint32_t index)
{
    Pair p;
    for (int i = 0; i < 20; ++i) p.w[i] = g.u32();
    for (int a = 0; a < 3; ++a) p.w[a] = f2u(g.below(8) ? g.sym() : g.sym() * 1e30f);
    uint32_t e[3];
    for (int a = 0; a < 3; ++a) e[a] = g.below(6) ? 110u + g.below(20) : g.below(255); // any byte <= 254 now and then
    uint32_t imask = 0, meta[2] = { 0, 0 }, x = index;
    for (int k = 0; k < 8; ++k, x /= 3) {
        const uint32_t state = x % 3;
        if (state == 1) imask |= 1u << k;
        if (state == 2 || (state == 1 && g.below(2))) meta[k >> 2] |= (1u + g.below(255)) << (8 * (k & 3));
    }
    p.w[3] = e[0] | e[1] << 8 | e[2] << 16 | imask << 24;
    p.w[6] = meta[0];
    p.w[7] = meta[1];
    const uint32_t shape = g.below(4);
    if (shape == 0) { // duplicated child boxes: equal minima
        const uint32_t src = g.below(8);
        for (int k = 0; k < 8; ++k)
            if (g.below(2))
                for (int r = 0; r < 6; ++r) {
                    const uint32_t b = qbyte(p.w, r, (int)src);
                    uint32_t&      t = p.w[8 + 2 * r + (k >> 2)];
                    t = (t & ~(0xffu << (8 * (k & 3)))) | b << (8 * (k & 3));
                }
    } else if (shape == 1) { // zero-extent boxes: hi = lo
        for (int r = 0; r < 3; ++r) { p.w[14 + 2 * r] = p.w[8 + 2 * r]; p.w[15 + 2 * r] = p.w[9 + 2 * r]; }
    }
    for (int r = 0; r < 3; ++r) // lo <= hi: the bytes of the three upper rows raised to the lower rows'
        for (int h = 0; h < 2; ++h)
            for (int b = 0; b < 4; ++b) {
                const uint32_t lo = (p.w[8 + 2 * r + h] >> (8 * b)) & 0xffu, hi = (p.w[14 + 2 * r + h] >> (8 * b)) & 0xffu;
                if (hi < lo) p.w[14 + 2 * r + h] = (p.w[14 + 2 * r + h] & ~(0xffu << (8 * b))) | lo << (8 * b);
            }
    if (g.below(16) == 0) {
        if (g.below(2)) p.w[3] |= 0xffu << (8 * g.below(3));
        else { const uint32_t r = g.below(3), h = g.below(2); std::swap(p.w[8 + 2 * r + h], p.w[14 + 2 * r + h]); }
    }
    make_ray(p, g);
    p.filter = g.below(3) ? 0xffu : g.u32();
    return p;
}

Pair make_pair_at(const std::vector<uint32_t>& nodes, Rng& g, uint64_t i)
{
    return (i & 1) ? synthetic_pair(g, (uint32_t)(i >> 1)) : real_pair(nodes, g);
}

void words(const spw::Visit& v, uint32_t* out)
{
    out[0] = v.inner; out[1] = v.leaf; out[2] = (uint32_t)v.nearest; out[3] = f2u(v.t_rest);
}
spw::Visit general(const Pair& p) { return spw::visit<false>(p.w, p.o[0], p.o[1], p.o[2], p.inv[0], p.inv[1], p.inv[2], p.tmin, p.tmax, p.filter); }
spw::Visit plain(const Pair& p) { return spw::visit_plain(p.w, p.o[0], p.o[1], p.o[2], p.inv[0], p.inv[1], p.inv[2], p.tmin, p.tmax, p.filter); }
// the contract's equality: three words exactly, t_rest as a float value (a zero's sign is free)
bool same(const spw::Visit& a, const spw::Visit& b)
{
    return a.inner == b.inner && a.leaf == b.leaf && a.nearest == b.nearest && a.t_rest == b.t_rest;
}

struct Count {
    uint64_t in = 0, bad = 0, first = 0, nan_in = 0;
    uint64_t inner = 0, leaf = 0, second = 0, equal_min = 0, in_plane = 0, zero_dist = 0, overflow = 0, tmax_inf = 0, neg[3] = { 0, 0, 0 };
    uint64_t zero_sign = 0; // inside the contract: t_rest +0 against -0 (allowed, reported)
    uint64_t out = 0, out_differ = 0;
    Pair     first_pair;
    void add(const Count& c)
    {
        in += c.in; bad += c.bad; nan_in += c.nan_in; inner += c.inner; leaf += c.leaf; second += c.second; equal_min += c.equal_min;
        in_plane += c.in_plane; zero_dist += c.zero_dist; overflow += c.overflow; tmax_inf += c.tmax_inf;
        for (int a = 0; a < 3; ++a) neg[a] += c.neg[a];
        zero_sign += c.zero_sign; out += c.out; out_differ += c.out_differ;
    }
};

// what a pair inside the contract exercises, from the general form's own arithmetic restated per slot
void classify(const Pair& p, const spw::Visit& v, Count& c)
{
    c.inner += v.inner != 0;
    c.leaf += v.leaf != 0;
    c.second += (v.inner & (v.inner - 1)) != 0 && v.t_rest != spm::k_infinite;
    c.tmax_inf += p.tmax == INF;
    for (int a = 0; a < 3; ++a) c.neg[a] += p.inv[a] < 0.0f;
    const uint32_t valid = valid_slots(p.w, p.filter);
    bool  plane = false, zero = false, over = false, nan = false;
    float e[8];
    for (int k = 0; k < 8; ++k) {
        e[k] = QNAN;
        if (!((valid >> k) & 1u)) continue;
        float t0 = p.tmin;
        for (int a = 0; a < 3; ++a) {
            const float lo = decoded(p.w, a, k), hi = decoded(p.w, 3 + a, k);
            const float dn = lo - p.o[a], df = hi - p.o[a], tn = dn * p.inv[a], tf = df * p.inv[a];
            plane |= dn == 0.0f || df == 0.0f;
            zero |= tn == 0.0f || tf == 0.0f;
            over |= (std::isinf(tn) && std::isfinite(dn)) || (std::isinf(tf) && std::isfinite(df));
            nan |= tn != tn || tf != tf;
            const float n = tn < tf ? tn : tf;
            t0 = n > t0 ? n : t0;
        }
        if ((v.inner >> k) & 1u) e[k] = t0;
    }
    bool eq = false;
    for (int k = 0; k < 8; ++k)
        for (int j = k + 1; j < 8; ++j) eq |= e[k] == e[j]; // NaN marks a slot that is no hit inner child
    c.equal_min += eq;
    c.in_plane += plane;
    c.zero_dist += zero;
    c.overflow += over;
    c.nan_in += nan;
}

// the predicate on its own: what it must reject and what it must keep
int predicate_failures()
{
    int bad = 0;
    const float ok[8] = { 0.5f, -2.0f, 1e30f, 3.0f, -1e-30f, 1e38f, 0.0f, INF };
    bad += !spw::plain_ray(ok[0], ok[1], ok[2], ok[3], ok[4], ok[5], ok[6], ok[7]);
    bad += !spw::plain_ray(0.0f, -0.0f, 1e-40f, 1e-40f, -3.0e38f, 1.0f, -0.0f, 3.0e38f); // zero and denormal origins, a denormal inverse
    bad += !spw::plain_ray(0.0f, 0.0f, 0.0f, 1.0f, 1.0f, 1.0f, -INF, INF);
    for (int j = 0; j < 8; ++j) {
        std::vector<float> rej;
        if (j < 3) rej = { INF, -INF, QNAN };
        else if (j < 6) rej = { INF, -INF, 0.0f, -0.0f, QNAN };
        else rej = { QNAN, -QNAN };
        for (float r : rej) {
            float v[8];
            std::memcpy(v, ok, sizeof v);
            v[j] = r;
            bad += spw::plain_ray(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]);
        }
    }
    return bad;
}

// the structural checker (sph::check_wide) on the node side of the contract: a clean tree has no
// error; a lower byte above its upper byte on an occupied slot, or a scale byte of 255, is kind 10
int checker_failures()
{
    Rng g{ 5 };
    std::vector<PrimBounds> b;
    for (int i = 0; i < 300; ++i) b.push_back(box(g.sym(), g.sym(), g.sym(), 0.01f + 0.03f * g.unit()));
    const sph::Bvh     bvh  = sph::build_bvh_sah(b, 2);
    const sph::WideBvh wide = sph::build_wide(bvh);
    int bad = sph::check_wide(wide, bvh.prim_order, b).errors != 0;
    std::printf("clean tree: %s\n", bad ? "FAILED" : "ok");
    {
        sph::WideBvh    t = wide;
        uint32_t*       w = t.words.data();
        const uint32_t  valid = valid_slots(w, 0xffu);
        bool            done = false;
        for (int k = 0; k < 8 && !done; ++k)
            for (int a = 0; a < 3 && !done; ++a)
                if (((valid >> k) & 1u) && qbyte(w, a, k) < qbyte(w, 3 + a, k)) {
                    const uint32_t lo = qbyte(w, a, k), hi = qbyte(w, 3 + a, k), sh = 8 * (k & 3);
                    uint32_t &     wl = w[8 + 2 * a + (k >> 2)], &wh = w[14 + 2 * a + (k >> 2)];
                    wl = (wl & ~(0xffu << sh)) | hi << sh;
                    wh = (wh & ~(0xffu << sh)) | lo << sh;
                    done = true;
                }
        const sph::WideCheck c  = sph::check_wide(t, bvh.prim_order, b);
        const bool           ok = done && c.errors > 0 && c.first_error_kind == sph::WIDE_ERR_QUANT;
        std::printf("planted swapped bytes: errors %lld kind %d %s\n", (long long)c.errors, c.first_error_kind, ok ? "ok" : "FAILED");
        bad += !ok;
    }
    {
        sph::WideBvh t = wide;
        t.words[3] |= 0xff00u;
        const sph::WideCheck c  = sph::check_wide(t, bvh.prim_order, b);
        const bool           ok = c.errors > 0 && c.first_error_kind == sph::WIDE_ERR_QUANT;
        std::printf("planted scale byte: errors %lld kind %d %s\n", (long long)c.errors, c.first_error_kind, ok ? "ok" : "FAILED");
        bad += !ok;
    }
    return bad;
}

// 600 triangles under a tree several wide levels deep, and four waves of rays: plain ones; plain ones
// but for one lane with d.y = 0 that starts in a box plane; axis-parallel ones; rays that start exactly
// in decoded planes of the root's children and run in plain directions.  Every ray stays inside what
// the render walks (NAN_SAFE = false) are defined for, DESIGN.md §24b: t_max is FLT_MAX or finite,
// never +inf, and no ray with d.z = 0 starts exactly in a z plane of any box -- such a ray can leave a
// hit node without a nearest child (an entry distance of +inf or NaN is not below FLT_MAX), which the
// integrators' rays never do and only the query kernels' NAN_SAFE walks handle.
int dump_walk(const char* path)
{
    Rng g{ 77 };
    const int NT = 600, NR = 256;
    std::vector<float>      tri((size_t)NT * 9);
    std::vector<PrimBounds> b((size_t)NT);
    for (int i = 0; i < NT; ++i) {
        const float c[3] = { g.sym(), g.sym(), 0.6f * g.sym() };
        for (int a = 0; a < 3; ++a) { b[(size_t)i].lo[a] = INF; b[(size_t)i].hi[a] = -INF; }
        for (int v = 0; v < 3; ++v)
            for (int a = 0; a < 3; ++a) {
                const float x = c[a] + 0.08f * g.sym();
                tri[(size_t)i * 9 + (size_t)v * 3 + (size_t)a] = x;
                b[(size_t)i].lo[a] = std::min(b[(size_t)i].lo[a], x);
                b[(size_t)i].hi[a] = std::max(b[(size_t)i].hi[a], x);
            }
    }
    const sph::Bvh     bvh  = sph::build_bvh_sah(b, 2);
    const sph::WideBvh wide = sph::build_wide(bvh);
    if (sph::check_wide(wide, bvh.prim_order, b).errors != 0) return 2;
    const uint32_t* root = wide.words.data();
    std::vector<float> rays((size_t)NR * 8);
    for (int r = 0; r < NR; ++r) {
        const int wave = r / 64, lane = r % 64;
        float     o[3] = { 0.3f * g.sym(), 0.3f * g.sym(), 3.2f }, d[3];
        if (g.below(3) == 0) for (int a = 0; a < 3; ++a) o[a] = 2.0f * g.nz(); // from all around
        auto aim_at = [&] { for (int a = 0; a < 3; ++a) { d[a] = 0.9f * g.sym() - o[a]; if (d[a] == 0.0f) d[a] = 0.125f; } };
        aim_at();
        if (wave == 1 && lane == 17) {
            o[1] = decoded(root, 1, (int)g.below(8));
            d[1] = 0.0f;
        } else if (wave == 2) {
            const int a = lane % 3;
            for (int j = 0; j < 3; ++j) { o[j] = 0.9f * g.sym(); d[j] = 0.0f; }
            o[a] = (lane & 4) ? 3.0f : -3.0f;
            d[a] = (lane & 4) ? -1.0f : 1.0f;
            const int p = a == 1 ? 0 : (a + 1) % 3; // x or y: a NaN slab distance there is replaced on the next axis
            if (lane & 8) o[p] = decoded(root, p, (int)g.below(8)); // in a plane it runs along
            if (a != 2) // d.z = 0: off every z plane of the tree
                for (bool clear = false; !clear;) {
                    clear = true;
                    for (size_t n = 0; n < wide.words.size() / 20 && clear; ++n)
                        for (int k = 0; k < 8 && clear; ++k)
                            clear = o[2] != decoded(&wide.words[20 * n], 2, k) && o[2] != decoded(&wide.words[20 * n], 5, k);
                    if (!clear) o[2] = 0.9f * g.sym();
                }
        } else if (wave == 3) {
            const int k = (int)g.below(8), n = 1 + lane % 3;
            for (int j = 0; j < n; ++j) o[(lane + j) % 3] = decoded(root, (g.below(2) ? 3 : 0) + (lane + j) % 3, k);
            aim_at();
        }
        float* q = &rays[(size_t)r * 8];
        q[0] = o[0]; q[1] = o[1]; q[2] = o[2]; q[3] = (lane & 1) ? 0.001f : 0.0f;
        q[4] = d[0]; q[5] = d[1]; q[6] = d[2]; q[7] = lane % 5 == 1 ? 0.8f + g.unit() : 3.40282346638528859812e+38f;
    }
    // the guard for the above: at no node of the tree, walked or not, may a ray hit inner children and
    // be given no nearest one (t_max only falls during a walk, which can only take hits away)
    for (int r = 0; r < NR; ++r) {
        const float* q = &rays[(size_t)r * 8];
        for (size_t n = 0; n < wide.words.size() / 20; ++n) {
            uint32_t w[20];
            std::memcpy(w, &wide.words[20 * n], 80);
            const spw::Visit v = spw::visit<false>(w, q[0], q[1], q[2], 1.0f / q[4], 1.0f / q[5], 1.0f / q[6], q[3], q[7], 0xffu);
            if (v.inner != 0u && (v.nearest < 0 || !((v.inner >> v.nearest) & 1u))) {
                std::printf("walk: ray %d has no nearest child at node %zu\n", r, n);
                return 2;
            }
        }
    }
    std::vector<float> rec(wide.slot_of.size() * 12);
    for (size_t ws = 0; ws < wide.slot_of.size(); ++ws) {
        const int32_t p = bvh.prim_order[(size_t)wide.slot_of[ws]];
        const float*  t = &tri[(size_t)p * 9];
        const float   code = u2f((uint32_t)p); // a triangle's code is its index
        const float   r12[12] = { t[0], t[1], t[2], code, t[3], t[4], t[5], 0.0f, t[6], t[7], t[8], 0.0f };
        std::memcpy(&rec[ws * 12], r12, sizeof r12);
    }
    const uint32_t head[4] = { (uint32_t)(wide.words.size() / 20), (uint32_t)wide.slot_of.size(), (uint32_t)wide.depth, (uint32_t)NR };
    FILE* f = std::fopen(path, "wb");
    if (!f) return 2;
    const bool ok = std::fwrite(head, 4, 4, f) == 4 && std::fwrite(wide.words.data(), 4, wide.words.size(), f) == wide.words.size() &&
                    std::fwrite(rec.data(), 4, rec.size(), f) == rec.size() && std::fwrite(rays.data(), 4, rays.size(), f) == rays.size();
    if (std::fclose(f) != 0 || !ok) return 2;
    std::printf("walk: %u records, %u slots, depth %u, %u rays\n", head[0], head[1], head[2], head[3]);
    return 0;
}

void print_pair(const char* what, uint64_t i, const Pair& p)
{
    uint32_t a[4], b[4];
    words(general(p), a);
    words(plain(p), b);
    std::printf("pair %llu %s:\n  visit      ", (unsigned long long)i, what);
    for (int j = 0; j < 4; ++j) std::printf(" %08x", a[j]);
    std::printf("\n  visit_plain");
    for (int j = 0; j < 4; ++j) std::printf(" %08x", b[j]);
    std::printf("\n  node");
    for (int j = 0; j < 20; ++j) std::printf(" %08x", p.w[j]);
    std::printf("\n  o %a %a %a inv %a %a %a tmin %a tmax %a filter %08x\n", p.o[0], p.o[1], p.o[2], p.inv[0], p.inv[1], p.inv[2], p.tmin,
                p.tmax, p.filter);
}

} // namespace

int main(int argc, char** argv)
{
    if (argc == 3 && std::string(argv[1]) == "walk") return dump_walk(argv[2]);
    const std::vector<uint32_t> nodes = real_nodes();
    if (argc == 5 && std::string(argv[1]) == "dump") {
        const long n = std::atol(argv[2]);
        FILE *     fi = std::fopen(argv[3], "wb"), *fo = std::fopen(argv[4], "wb");
        if (n <= 0 || !fi || !fo) return 2;
        Rng g{ 4242 };
        long done = 0;
        for (uint64_t i = 0; done < n; ++i) {
            const Pair p = make_pair_at(nodes, g, i);
            if (!ray_plain(p) || !node_in_contract(p)) continue;
            uint32_t row[32] = { 0 }, out[4];
            std::memcpy(row, p.w, 80);
            std::memcpy(row + 20, p.o, 12);
            std::memcpy(row + 23, p.inv, 12);
            std::memcpy(row + 26, &p.tmin, 4);
            std::memcpy(row + 27, &p.tmax, 4);
            row[28] = p.filter;
            words(general(p), out);
            if (std::fwrite(row, 4, 32, fi) != 32 || std::fwrite(out, 4, 4, fo) != 4) return 2;
            ++done;
        }
        if (std::fclose(fi) != 0 || std::fclose(fo) != 0) return 2;
        std::printf("dumped %ld pairs\n", n);
        return 0;
    }
    const uint64_t total = argc == 2 ? (uint64_t)std::atoll(argv[1]) : 16000000ull;
    const int      bad_pred = predicate_failures() + checker_failures();
    std::printf("plain_ray: %s\n", bad_pred ? "FAILED" : "ok");
    const uint64_t           BLOCK = 1u << 14, blocks = (total + BLOCK - 1) / BLOCK;
    const unsigned           nt = std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    std::vector<Count>       counts(nt);
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < nt; ++t)
        pool.emplace_back([&, t] {
            Count& c = counts[t];
            for (uint64_t blk = t; blk < blocks; blk += nt) {
                Rng            g{ 4242 + blk };
                const uint64_t end = std::min(total, (blk + 1) * BLOCK);
                for (uint64_t i = blk * BLOCK; i < end; ++i) {
                    const Pair       p = make_pair_at(nodes, g, i);
                    const spw::Visit a = general(p), b = plain(p);
                    if (!ray_plain(p)) { // outside: the forms may differ, and somewhere they must
                        ++c.out;
                        c.out_differ += !same(a, b);
                        continue;
                    }
                    if (!node_in_contract(p)) continue;
                    ++c.in;
                    classify(p, a, c);
                    c.zero_sign += f2u(a.t_rest) != f2u(b.t_rest) && a.t_rest == b.t_rest;
                    if (!same(a, b)) {
                        if (c.bad == 0) { c.first = i; c.first_pair = p; }
                        ++c.bad;
                    }
                }
            }
        });
    for (auto& th : pool) th.join();
    Count s;
    for (const Count& c : counts) {
        s.add(c);
        if (c.bad) print_pair("differs inside the contract", c.first, c.first_pair);
    }
    std::printf("%llu pairs (%zu real nodes): %llu inside the contract, %llu rejected rays\n", (unsigned long long)total, nodes.size() / 20,
                (unsigned long long)s.in, (unsigned long long)s.out);
    std::printf("inside: inner %llu leaf %llu second %llu equal_min %llu in_plane %llu zero_dist %llu overflow %llu tmax_inf %llu "
                "neg_x %llu neg_y %llu neg_z %llu zero_sign %llu nan %llu\n",
                (unsigned long long)s.inner, (unsigned long long)s.leaf, (unsigned long long)s.second, (unsigned long long)s.equal_min,
                (unsigned long long)s.in_plane, (unsigned long long)s.zero_dist, (unsigned long long)s.overflow,
                (unsigned long long)s.tmax_inf, (unsigned long long)s.neg[0], (unsigned long long)s.neg[1], (unsigned long long)s.neg[2],
                (unsigned long long)s.zero_sign, (unsigned long long)s.nan_in);
    std::printf("rejected: %llu differ\n", (unsigned long long)s.out_differ);
    std::printf("%llu failing\n", (unsigned long long)(s.bad + (uint64_t)bad_pred + s.nan_in));
    return (s.bad || bad_pred || s.nan_in) ? 1 : 0;
}
