// nee_black_main.cpp -- spn::nee_black_known (simplepath_amd/csrc/common/sp_nee_black.h) against what it
// stands for: cblack of the finishing expression, for the weights that glossy_weights would make of
// ANY estimate luminance in [0, k_est_max].  Every table value says by hand whether it lies inside
// its guard face; the decider may answer "unknown" only where some value lies outside.
//   nee_black_main [stride]   stride > 1 thins the table sweep (the sanitizer run)
#include "../../simplepath_amd/csrc/common/sp_nee_black.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

using namespace spn;

struct V {
    float v;
    bool  in;
};
static float up(float x) { return std::nextafter(x, std::numeric_limits<float>::infinity()); }
static float dn(float x) { return std::nextafter(x, -std::numeric_limits<float>::infinity()); }
static const float INF = std::numeric_limits<float>::infinity(), QNAN = std::numeric_limits<float>::quiet_NaN();
static const float SUB = std::numeric_limits<float>::denorm_min();

struct Counts {
    unsigned long long cases = 0, in_box = 0, unknown = 0, unknown_in_box = 0, black = 0, not_black = 0, wrong = 0;
};

static void one(Counts& n, bool bounded, float P, rgb E, rgb albedo, float A, bool coat, float cf, bool inside,
                const std::vector<float>& est)
{
    const int k = nee_black_known(bounded, P, E, albedo, A, coat, cf);
    ++n.cases;
    n.in_box += inside;
    if (k == NEE_UNKNOWN) {
        ++n.unknown;
        if (inside) {
            if (n.unknown_in_box++ < 10)
                std::printf("unknown inside the box: P %a E %a %a %a albedo %a %a %a A %a coat %d cf %a\n", P, E.r, E.g, E.b,
                            albedo.r, albedo.g, albedo.b, A, (int)coat, cf);
        }
        return;
    }
    (k == NEE_BLACK ? n.black : n.not_black)++;
    for (float r0 : est) {
        float w[2];
        weights_from(r0, A, w);
        const bool b = cblack(nee_finish(P, E, albedo, w, coat, cf));
        if (b != (k == NEE_BLACK)) {
            if (n.wrong++ < 10)
                std::printf("WRONG: decider %d, f black %d: est %a P %a E %a %a %a albedo %a %a %a A %a coat %d cf %a\n", k, (int)b,
                            r0, P, E.r, E.g, E.b, albedo.r, albedo.g, albedo.b, A, (int)coat, cf);
        }
    }
}

int main(int argc, char** argv)
{
    const unsigned stride = argc > 1 ? (unsigned)std::atoi(argv[1]) : 1u;
    const std::vector<float> est = { 0.0f, SUB, 1e-38f, 1e-10f, 1e-3f, 0.05f, 0.5f, 1.0f, 10.0f, 1e4f, 0x1p24f, dn(k_est_max), k_est_max };
    const std::vector<V> Ps = { { 0.0f, true }, { -0.0f, true }, { SUB, true }, { 1e-38f, true }, { 1e-3f, true }, { 1.0f, true },
                                { 6.7f, true }, { dn(k_pe_max), true }, { k_pe_max, true }, { up(k_pe_max), false },
                                { INF, false }, { QNAN, false }, { -SUB, false }, { -1.0f, false } };
    const std::vector<V> As = { { k_lum_min, true }, { dn(k_lum_min), false }, { 0.0f, false }, { SUB, false }, { 0.6f, true },
                                { 1.0f, true }, { k_lum_max, true }, { up(k_lum_max), false }, { QNAN, false }, { INF, false },
                                { -1.0f, false } };
    // albedo channel values; "in": inside [0, k_albedo_max]; the top-channel face is judged per triple
    const std::vector<V> Cs = { { 0.0f, true }, { -0.0f, true }, { SUB, true }, { dn(k_albedo_top_min), true }, { k_albedo_top_min, true },
                                { 0.19f, true }, { 1.0f, true }, { k_albedo_max, true }, { up(k_albedo_max), false },
                                { QNAN, false }, { -SUB, false }, { INF, false } };
    struct Coat { bool coat; float cf; bool in; };
    const std::vector<Coat> Fs = { { false, 1.0f, true }, { true, 0.0f, true }, { true, -0.0f, true }, { true, k_coat_min, true },
                                   { true, dn(k_coat_min), false }, { true, SUB, false }, { true, 1e-3f, true }, { true, 0.5f, true },
                                   { true, 1.0f, true }, { true, k_coat_max, true }, { true, up(k_coat_max), false },
                                   { true, QNAN, false }, { true, INF, false }, { true, -k_coat_min, true }, { true, -0.5f, true },
                                   { true, -dn(k_coat_min), false } };
    Counts   n;
    unsigned tick = 0;
    for (const V& P : Ps)
        for (const V& e : Ps) // mf_eval's channels share mf_pdf's faces
            for (int ep = 0; ep < 3; ++ep)
                for (const V& a : Cs)
                    for (int ap = 0; ap < 3; ++ap)
                        for (const V& A : As)
                            for (const Coat& F : Fs) {
                                if (++tick % stride) continue;
                                const rgb E   = ep == 0 ? mkc(e.v, e.v, e.v) : ep == 1 ? mkc(e.v, 0.0f, 0.0f) : mkc(0.0f, 1.0f, e.v);
                                const rgb alb = ap == 0 ? mkc(a.v, a.v, a.v) : ap == 1 ? mkc(0.0f, a.v, 0.0f) : mkc(a.v, 0.0f, SUB);
                                const bool top = a.v >= k_albedo_top_min; // a NaN is not
                                const bool inside = P.in && e.in && a.in && top && A.in && F.in;
                                one(n, true, P.v, E, alb, A.v, F.coat, F.cf, inside, est);
                                // a lane outside the estimate's guard never gets an answer
                                if (nee_black_known(false, P.v, E, alb, A.v, F.coat, F.cf) != NEE_UNKNOWN) ++n.wrong;
                            }
    std::printf("tables: %llu cases, %llu inside the box, %llu unknown (%llu inside the box), %llu black, %llu not black\n", n.cases,
                n.in_box, n.unknown, n.unknown_in_box, n.black, n.not_black);

    // random points of the box, log-uniform, with A as the device forms it
    Counts       m;
    std::mt19937 g(12345);
    auto logu = [&](float lo, float hi) { return std::exp2(std::uniform_real_distribution<float>(std::log2(lo), std::log2(hi))(g)); };
    const unsigned long long rnd = 2000000ull / stride;
    for (unsigned long long i = 0; i < rnd; ++i) {
        const float P   = (g() & 7u) ? logu(1e-30f, k_pe_max) : 0.0f;
        const rgb   E   = mkc((g() & 3u) ? logu(1e-30f, k_pe_max) : 0.0f, (g() & 3u) ? logu(1e-30f, k_pe_max) : 0.0f, logu(1e-30f, k_pe_max));
        const rgb   alb = mkc(logu(k_albedo_top_min, 4.0f), (g() & 1u) ? 0.0f : logu(1e-20f, 4.0f), logu(1e-20f, 4.0f));
        const float A   = lambert_lum(alb);
        if (!(A >= k_lum_min && A <= k_lum_max)) continue;
        const unsigned c = g() % 4u;
        const float cf = c == 0 ? 1.0f : c == 1 ? 0.0f : logu(k_coat_min, 1.0f);
        std::vector<float> e1 = { (g() & 1u) ? logu(1e-30f, k_est_max) : logu(1e-3f, 4.0f) };
        one(m, true, P, E, alb, A, c != 0, cf, true, e1);
    }
    std::printf("random: %llu cases, %llu unknown, %llu black, %llu not black\n", m.cases, m.unknown, m.black, m.not_black);
    std::printf("%llu unknown inside the box\n", n.unknown_in_box + m.unknown_in_box);
    std::printf("%llu failing\n", n.wrong + m.wrong);
    return (n.wrong + m.wrong + n.unknown_in_box + m.unknown_in_box) ? 1 : 0;
}
