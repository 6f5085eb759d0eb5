// nee_order_units.hip -- direct_nee (sp_path.hpp: the shadow ray first, the glossy estimate skipped
// where the sample is occluded) beside the order it replaced, which is kept in this
// file only, as the specification: Light::sample, Material::eval, then the shadow ray where f is not
// black.  One wave per case; every lane runs both forms on the same hit, the same wo and two equal
// streams, and a third stream replays the decisions (usable, occluded, what the decider says, where
// the estimate starts) so that tests/test_gpu_nee_order.py can tell which path a lane took.
//   nee_order_units <rsqrt_table.bin> <out.bin>      (built once per SP_NEE_SKIP form, nee_order.mk)
// The scene: the plane y = 0 is where the hits lie (not a shape: the hits are given), one sphere
// of radius 1 at (0, 1.5, 0) occludes, sphere lights of radius 0.3 at (0, 4, 0) and (3, 3, 2).
// out: CASES x 64 lanes x 32 words -- new form {L 3, shadow, rays, draws, idx, cur, ready, the next
// two numbers of the stream} at 0, the old form's at 11, then per light 4 bits {usable, occluded,
// decider 2} at 22, wo.y in the shading frame at 23, the stream index where the first estimate
// starts at 24 (~0: none); an inactive lane keeps the fill 0xeeeeeeee.
// Exit 2: bad arguments or files; exit 3: a HIP error (nothing is launched after one).
#define SP_RNG_PF 0 // the DirectLighting megakernel's stream options (sp_mega_direct.hip)
#define SP_RHO_TOUCH 1
#define SP_RNG_PAIR 1
#include "sp_path.hpp"
#include "sp_rsqrt_pack.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace spd;
using namespace spm;

namespace {

constexpr int IN = 16, OUT = 32, FORM = 11, CASES = 9;

#define HIP_OK(expr)                                                                                                   \
    do {                                                                                                               \
        const hipError_t e_ = (expr);                                                                                  \
        if (e_ != hipSuccess) {                                                                                        \
            std::fprintf(stderr, "nee_order_units: %s: %s\n", #expr, hipGetErrorString(e_));                           \
            std::exit(3);                                                                                              \
        }                                                                                                              \
    } while (0)

// DirectLightingIntegrator::do_integrate's light loop in the reference's order (Integrator.cpp:302-304)
__device__ __forceinline__ rgb direct_nee_old(Ctx& c, const Isect& is, f3 wo)
{
    rgb L = mkc(0, 0, 0);
    for (int li = 0; li < c.sc.n_lights; ++li) {
        const Light   l  = uload_light(c.sc.lights + li);
        const LSample ls = light_sample(c.sc, l, is.p, is.n, next2D(c.rng), c.q);
        if (ls.pdf == 0.0f || cblack(ls.L)) continue;
        const f3  wi  = ls.ray.d;
        const rgb f   = material_eval(c.sc, is.material, wo, wi, is.n, c.rng, c.q);
        bool      vis = false;
        if (!cblack(f)) vis = !occluded(c, ls.ray, ls.tmin, ls.tmax);
        if (vis) L = cadd(L, cdivs(cscale(cmul(f, ls.L), abs_f(dot(wi, is.n))), ls.pdf));
    }
    return L;
}

__device__ __forceinline__ void put_form(uint32_t* o, rgb L, const Ctx& c, Rng& r)
{
    o[0] = __float_as_uint(L.r); o[1] = __float_as_uint(L.g); o[2] = __float_as_uint(L.b);
    o[3] = c.shadow; o[4] = c.rays; o[5] = r.draws; o[6] = (uint32_t)r.idx; o[7] = (uint32_t)r.cur; o[8] = (uint32_t)r.ready;
    o[9]  = __float_as_uint(next1D(r)); // what the next Light::sample would read
    o[10] = __float_as_uint(next1D(r));
}

// in: per lane {p 3, n 3, wo 3, material, seed, skip, active, lights, prepare, 0}
__global__ __launch_bounds__(64) void nee_kernel(Scene sc, const uint32_t* __restrict__ table, int table_words,
                                                 const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint64_t* state)
{
    extern __shared__ uint32_t lds[];
    const int lane = threadIdx.x;
    for (int i = lane; i < table_words; i += 64) lds[i] = table[i];
    libm_lds_init(lane, 64);
    __syncthreads();
    const Rsq   q{ lds };
    const Stack st{ lds + table_words, lane, 1 }; // no BVH in this scene: never pushed to
    const uint32_t* w = in + ((size_t)blockIdx.x * 64 + lane) * IN;
    uint32_t*       o = out + ((size_t)blockIdx.x * 64 + lane) * OUT;
    Scene s    = sc;
    s.n_lights = (int)w[13];
    Isect is;
    is.t = 1.0f;
    is.p = mk(__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2]));
    is.n = mk(__uint_as_float(w[3]), __uint_as_float(w[4]), __uint_as_float(w[5]));
    is.material = (int)w[9];
    const f3 wo = mk(__uint_as_float(w[6]), __uint_as_float(w[7]), __uint_as_float(w[8]));
    Rng rng[3]; // the new form's stream, the old form's, the replay's: equal
    for (int k = 0; k < 3; ++k) {
        rng[k].base = state + ((size_t)blockIdx.x * 3 + k) * (2 * (size_t)MT_GEN_WORDS) + (size_t)lane * MT_BLK;
        rng_seed(rng[k], w[10]);
        rng_skip(rng[k], (int)w[11]);
        if (w[14]) rng_prepare(rng[k]); // the whole wave, as the kernels call it at a sample's start
        rng[k].draws = 0; // counted from here
    }
    if (!w[12]) return; // divergent entry: only some lanes hold a geometry hit
    {
        Ctx       c{ s, rng[0], q, st, 0u, 0u };
        const rgb L = direct_nee(c, is, wo);
        put_form(o, L, c, rng[0]);
    }
    {
        Ctx       c{ s, rng[1], q, st, 0u, 0u };
        const rgb L = direct_nee_old(c, is, wo);
        put_form(o + FORM, L, c, rng[1]);
    }
    // the replay: what each light's sample is, on a stream that moves as the old form's does
    Rng&            r    = rng[2];
    const Material& m    = s.materials[is.material];
    const bool      coat = m.kind == SP_MAT_CLEARCOAT;
    const Material& mb   = s.materials[coat ? m.base : is.material];
    const bool      rho  = mb.kind != SP_MAT_LAMBERTIAN;
    const Onb       ob   = onb_from_v(is.n, q);
    const f3        wol  = to_onb(ob, wo);
    uint32_t flags = 0u, first = 0xffffffffu;
    for (int li = 0; li < s.n_lights; ++li) {
        const Light   l  = uload_light(s.lights + li);
        const LSample ls = light_sample(s, l, is.p, is.n, next2D(r), q);
        if (ls.pdf == 0.0f || cblack(ls.L)) continue;
        const f3    wil = to_onb(ob, ls.ray.d);
        const bool  occ = scene_any(s, ls.ray, ls.tmin, ls.tmax, st);
        const float cf  = coat ? 1.0f - fresnel_dielectric(wol.y, 1.0f, m.coat_ior) : 1.0f;
        int         known = 3; // no estimate
        if (rho) {
            known = spn::nee_black_known(
                spn::estimate_bounded(wol, mb.alpha_x, mb.alpha_y, mb.microfacet_ior, mb.microfacet_r, mb.sample_visible_area != 0),
                mf_pdf(mb, wol, wil, q), mf_eval(mb, wol, wil, q), mb.lambert_albedo, spn::lambert_lum(mb.lambert_albedo), coat, cf);
            if (first == 0xffffffffu) first = (uint32_t)r.idx;
            rng_reserve(r, 32);
            if (wol.y != 0.0f) rng_skip_reserved(r, 32);
        }
        flags |= (1u | (occ ? 2u : 0u) | ((uint32_t)known << 2)) << (4 * li);
    }
    o[22] = flags;
    o[23] = __float_as_uint(wol.y);
    o[24] = first;
}

int fail(const char* msg)
{
    std::fprintf(stderr, "nee_order_units: %s\n", msg);
    return 2;
}

aff sphere_o2w(float r, float x, float y, float z) { aff a; a.vx = mk(r, 0, 0); a.vy = mk(0, r, 0); a.vz = mk(0, 0, r); a.p = mk(x, y, z); return a; }
aff sphere_w2o(float r, float x, float y, float z) { aff a; a.vx = mk(1 / r, 0, 0); a.vy = mk(0, 1 / r, 0); a.vz = mk(0, 0, 1 / r); a.p = mk(-x / r, -y / r, -z / r); return a; }

Material glossy(float alpha, float ior, float r, float g, float b)
{
    Material m = {};
    m.kind = SP_MAT_GLOSSY; m.base = -1;
    m.lambert_albedo = mkc(r / k_pi, g / k_pi, b / k_pi);
    m.microfacet_r   = mkc(1, 1, 1);
    m.alpha_x = m.alpha_y = alpha; m.microfacet_ior = ior;
    m.sample_visible_area = 1;
    return m;
}

f3 unit(double x, double y, double z)
{
    const double l = std::sqrt(x * x + y * y + z * z);
    return mk((float)(x / l), (float)(y / l), (float)(z / l));
}

template <class T>
T* to_device(const std::vector<T>& v)
{
    T* d = nullptr;
    HIP_OK(hipMalloc(&d, v.size() * sizeof(T)));
    HIP_OK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return d;
}

} // namespace

int main(int argc, char** argv)
{
    if (argc != 3) return fail("usage: nee_order_units <rsqrt_table.bin> <out.bin>");
    std::vector<uint32_t> t;
    {
        FILE* f = std::fopen(argv[1], "rb");
        if (!f) return fail("cannot open the table");
        std::fseek(f, 0, SEEK_END);
        const long bytes = std::ftell(f);
        std::fseek(f, 0, SEEK_SET);
        if (bytes < 16 || bytes % 4 != 0 || bytes > (1l << 20)) { std::fclose(f); return fail("the table file is no words"); }
        t.resize((size_t)bytes / 4);
        const size_t got = std::fread(t.data(), 4, t.size(), f);
        std::fclose(f);
        if (got != t.size() || t[0] < 1u || t[0] > 13u || t.size() != 3 + ((size_t)2 << t[0])) return fail("not bits, zero, denorm and 2 << bits entries");
    }
    const std::vector<uint32_t> table = rsqrt_device_words(t.data() + 3, t.size() - 3, (int32_t)t[0], t[1], t[2], true);
    if (table[3] == 0u) return fail("this host's RSQRTSS table does not pack to 16-bit entries");
    if (table.size() > 12000) return fail("the table does not fit the kernel's LDS");

    // materials: 0 glossy plane, 1 glossy base, 2 clearcoat over 1, 3 Lambertian
    std::vector<Material> mats(4);
    mats[0] = glossy(0.5f, 1.8f, 0.6f, 0.6f, 0.6f);
    mats[1] = glossy(0.35f, 1.8f, 0.8f, 0.2f, 0.8f);
    mats[2] = {};
    mats[2].kind = SP_MAT_CLEARCOAT; mats[2].base = 1; mats[2].coat_ior = 1.3f; mats[2].coat_color = mkc(1, 1, 1);
    mats[3] = {};
    mats[3].kind = SP_MAT_LAMBERTIAN; mats[3].base = -1; mats[3].lambert_albedo = mkc(0.1f / k_pi, 0.8f / k_pi, 0.8f / k_pi);
    std::vector<Shape> shapes(1);
    shapes[0] = {};
    shapes[0].o2w = sphere_o2w(1.0f, 0.0f, 1.5f, 0.0f);
    shapes[0].w2o = sphere_w2o(1.0f, 0.0f, 1.5f, 0.0f);
    shapes[0].nrm.vx = mk(1, 0, 0); shapes[0].nrm.vy = mk(0, 1, 0); shapes[0].nrm.vz = mk(0, 0, 1);
    shapes[0].material = 3; shapes[0].kind = SP_PRIM_SPHERE;
    std::vector<Light> lights(2);
    const float lp[2][3] = { { 0.0f, 4.0f, 0.0f }, { 3.0f, 3.0f, 2.0f } };
    for (int i = 0; i < 2; ++i) {
        lights[i] = {};
        lights[i].kind = SP_LIGHT_SPHERE; lights[i].image = -1;
        lights[i].radiance = i ? mkc(20, 10, 10) : mkc(40, 40, 40);
        lights[i].o2w = sphere_o2w(0.3f, lp[i][0], lp[i][1], lp[i][2]);
        lights[i].w2o = sphere_w2o(0.3f, lp[i][0], lp[i][1], lp[i][2]);
        lights[i].nrm.vx = mk(1 / 0.3f, 0, 0); lights[i].nrm.vy = mk(0, 1 / 0.3f, 0); lights[i].nrm.vz = mk(0, 0, 1 / 0.3f);
    }
    const std::vector<int32_t> unbounded = { 0 };

    std::vector<uint32_t> in((size_t)CASES * 64 * IN, 0u);
    auto fb = [](float f) { return __builtin_bit_cast(uint32_t, f); };
    for (int c = 0; c < CASES; ++c)
        for (int l = 0; l < 64; ++l) {
            uint32_t* w = &in[((size_t)c * 64 + l) * IN];
            const double a = 6.283185307179586 * l / 64.0;
            f3       p  = mk((float)(0.25 * std::cos(a)), 0.0f, (float)(0.25 * std::sin(a))); // in the umbra of light 0
            f3       wo = unit(0.3 + 0.01 * l, 1.0, 0.2);
            uint32_t mat = 0u, skip = 10u + (uint32_t)l, active = 1u, nl = 1u, prep = 0u;
            const f3 across = mk(-3.0f + 6.0f * (float)l / 63.0f, 0.0f, 0.1f); // umbra, penumbra and lit
            switch (c) {
            case 0: break;                                                       // every lane occluded
            case 1: p = across; break;                                           // a mixed wave
            case 2: if (l == 5 || l == 37) wo = unit(1.0, 1.0 / 4096.0, 0.1); break; // |wo.y| < 2^-10: unknown
            case 3: mat = 2u; p = mk(-2.5f + 5.0f * (float)l / 63.0f, 0.0f, 0.1f);   // the clearcoat from behind
                    if (l % 2 == 0) wo = unit(0.9, -0.3, 0.2);
                    break;
            case 4: if (l % 2) p = across;                                       // wo.y == 0: no draws
                    if (l % 4 == 0) wo = mk(1.0f, 0.0f, 0.0f);
                    break;
            case 5: nl = 2u; skip = (l < 32) ? 298u : 290u + (uint32_t)(l - 32); // the estimate starts at word 300 of 312
                    if (l % 2) p = across;
                    break;
            case 6: nl = 2u; skip = 298u; prep = 1u; if (l % 2) p = across; break;   // the same with the next generation ready
            case 7: nl = 2u; break;                                              // light 0 occluded, light 1 visible
            default: nl = 2u; p = across; active = (l % 3 != 0) ? 1u : 0u;       // divergent entry, three materials
                     mat = (l % 4 == 1) ? 3u : (l % 4 == 2) ? 2u : 0u;
                     break;
            }
            w[0] = fb(p.x); w[1] = fb(p.y); w[2] = fb(p.z);
            w[3] = fb(0.0f); w[4] = fb(1.0f); w[5] = fb(0.0f);
            w[6] = fb(wo.x); w[7] = fb(wo.y); w[8] = fb(wo.z);
            w[9] = mat; w[10] = 1000u * (uint32_t)c + (uint32_t)l + 1u; w[11] = skip; w[12] = active; w[13] = nl; w[14] = prep;
        }

    Scene sc = {};
    sc.max_depth   = 1;
    sc.n_unbounded = 1;
    sc.unbounded   = to_device(unbounded);
    sc.shapes      = to_device(shapes);
    sc.n_lights    = 2;
    sc.lights      = to_device(lights);
    sc.materials   = to_device(mats);
    sc.stack_depth = 1;
    sc.stack_words = 1;
    uint32_t* d_table = to_device(table);
    uint32_t* d_in    = to_device(in);
    uint32_t* d_out   = nullptr;
    uint64_t* d_state = nullptr;
    const size_t out_words = (size_t)CASES * 64 * OUT, state_words = (size_t)CASES * 3 * 2 * (size_t)MT_GEN_WORDS;
    HIP_OK(hipMalloc(&d_out, out_words * 4));
    HIP_OK(hipMemset(d_out, 0xee, out_words * 4));
    HIP_OK(hipMalloc(&d_state, state_words * 8));
    HIP_OK(hipMemset(d_state, 0, state_words * 8));
    const size_t lds_bytes = (table.size() + 64) * 4;
    if (lds_bytes > 32768)
        HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(&nee_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    nee_kernel<<<CASES, 64, lds_bytes>>>(sc, d_table, (int)table.size(), d_in, d_out, d_state);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    std::vector<uint32_t> out(out_words);
    HIP_OK(hipMemcpy(out.data(), d_out, out_words * 4, hipMemcpyDeviceToHost));
    FILE* f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(out.data(), 4, out.size(), f) != out.size() || std::fclose(f) != 0) return fail("cannot write the output");
    std::printf("nee_order %d %d\n", CASES, SP_NEE_SKIP);
    return 0;
}
