// TEST PROGRAM: evaluates one device leaf function of the renderer on rows of the caller's choosing.
//
//   device_units <function> <in.bin> <out.bin> [rsqrt_table.bin [image.bin]]
//
// Built once per kernel option set (tests/cpp/Makefile SET_*: the #define SP_... preamble of a
// family of translation units, as -D flags), as _build/device_units and _build/device_units_<set>.
//
// in.bin holds n rows of k 32-bit words, out.bin receives n rows of m words (k and m per function:
// the table in tests/_units.py, restated in FUNCTIONS below).  One launch evaluates the function
// once per row.  Prints "function n kernel_ms".  The program holds no reference and judges
// nothing: tests/test_gpu_units.py compares the words with oracle/sp_oracle.c orc_unit.
// rsqrt_table.bin (functions that take an Rsq): bits, zero_result, denorm_result, 2 << bits entries,
// as sp_rsqrt_table_get returns them; it is put into the device form by the upload's own
// rsqrt_device_words and copied to LDS as the render kernels copy it.
//
// The kernel has the render kernels' shape: 256 threads (wave64), every thread takes part in
// libm_lds_init and the barrier before anything else, and it is compiled with the library's
// numeric and device flags (simplepath_amd/flags.mk).
#include "sp_path.hpp"
#include "sp_rsqrt_pack.hpp"
#include "../host/sp_host.hpp" // build_env_map, the upload's host builder of the image light's tables

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace spd;
using namespace spm;

namespace {

enum { RSQ_NONE = 0, RSQ_PACKED = 1, RSQ_U32 = 2 };

__device__ __forceinline__ float wf(const uint32_t* w, int i) { return __uint_as_float(w[i]); }
__device__ __forceinline__ f3    wv(const uint32_t* w, int i) { return mk(wf(w, i), wf(w, i + 1), wf(w, i + 2)); }
__device__ __forceinline__ void  put(uint32_t* o, int i, float f) { o[i] = __float_as_uint(f); }
__device__ __forceinline__ void  putv(uint32_t* o, int i, f3 v) { put(o, i, v.x); put(o, i + 1, v.y); put(o, i + 2, v.z); }
__device__ __forceinline__ P2    wp2(const uint32_t* w, int i) { P2 u; u.x = wf(w, i); u.y = wf(w, i + 1); return u; }
__device__ __forceinline__ Material unit_material(float ax, float ay, float ior)
{
    Material m;
    m.kind = 1; m.base = -1;
    m.lambert_albedo = mkc(0, 0, 0);
    m.microfacet_r   = mkc(1.0f, 0.5f, 0.25f);
    m.alpha_x = ax; m.alpha_y = ay; m.microfacet_ior = ior;
    m.sample_visible_area = 1;
    m.coat_ior   = 0.0f;
    m.coat_color = mkc(0, 0, 0);
    return m;
}
__device__ __forceinline__ RsqrtTable rsq_table(const Rsq& q) // as rsqrt_ref reads it (sp_path.hpp)
{
    const uint4    h  = *reinterpret_cast<const uint4*>(q.t);
    const uint32_t hi = q.t[4];
    return RsqrtTable{ q.t + RSQ_HDR, (int32_t)h.x, h.y, h.z, (int32_t)h.w, hi };
}

// One struct per function: K input words and M output words per row, which table form it needs,
// and the evaluation.  Rows that a test calls a miss leave their outputs zero.
#define UNIT(NAME, KK, MM, RSQ, ...)                                                                                   \
    struct NAME {                                                                                                      \
        static constexpr int K = KK, M = MM, TABLE = RSQ;                                                              \
        static __device__ __forceinline__ void eval(const uint32_t* w, uint32_t* o, const Rsq& q) { __VA_ARGS__ }      \
    };

// a. libm
UNIT(u_expf, 1, 1, RSQ_NONE, put(o, 0, lm_expf(wf(w, 0)));)
UNIT(u_logf, 1, 1, RSQ_NONE, put(o, 0, lm_logf(wf(w, 0)));)
UNIT(u_sinf, 1, 1, RSQ_NONE, put(o, 0, lm_sinf(wf(w, 0)));)
UNIT(u_cosf, 1, 1, RSQ_NONE, put(o, 0, lm_cosf(wf(w, 0)));)
UNIT(u_erff, 1, 1, RSQ_NONE, put(o, 0, lm_erff(wf(w, 0)));)
UNIT(u_acosf, 1, 1, RSQ_NONE, put(o, 0, lm_acosf(wf(w, 0)));)
UNIT(u_atanf, 1, 1, RSQ_NONE, put(o, 0, lm_atanf(wf(w, 0)));)
UNIT(u_fmod1, 1, 1, RSQ_NONE, put(o, 0, fmod1(wf(w, 0)));)
UNIT(u_roundf, 1, 1, RSQ_NONE, put(o, 0, round_f(wf(w, 0)));)
UNIT(u_sincosf, 1, 2, RSQ_NONE, float s, c; lm_sincosf(wf(w, 0), &s, &c); put(o, 0, s); put(o, 1, c);)
UNIT(u_sincosf_bounded, 1, 2, RSQ_NONE, float s, c; lm_sincosf_bounded(wf(w, 0), &s, &c); put(o, 0, s); put(o, 1, c);)
UNIT(u_powf, 2, 1, RSQ_NONE, put(o, 0, lm_powf(wf(w, 0), wf(w, 1)));)
UNIT(u_atan2f, 2, 1, RSQ_NONE, put(o, 0, lm_atan2f(wf(w, 0), wf(w, 1)));)
UNIT(u_powf_unit, 2, 2, RSQ_NONE, put(o, 0, lm_powf_unit(wf(w, 0), wf(w, 1))); put(o, 1, lm_powf(wf(w, 0), wf(w, 1)));)
// b. arithmetic under the build flags
UNIT(u_div, 2, 1, RSQ_NONE, put(o, 0, wf(w, 0) / wf(w, 1));)
UNIT(u_sqrt, 1, 1, RSQ_NONE, put(o, 0, sqrt_f(wf(w, 0)));)
UNIT(u_fma, 3, 1, RSQ_NONE, put(o, 0, fma_f(wf(w, 0), wf(w, 1), wf(w, 2)));)
UNIT(u_muladd, 3, 1, RSQ_NONE, const float p = wf(w, 0) * wf(w, 1); put(o, 0, p + wf(w, 2));) // must stay unfused
UNIT(u_sqrt_unit, 1, 1, RSQ_NONE, put(o, 0, sqrt_unit(wf(w, 0)));)
UNIT(u_dot, 6, 1, RSQ_NONE, put(o, 0, dot(wv(w, 0), wv(w, 3)));)
UNIT(u_cross, 6, 3, RSQ_NONE, putv(o, 0, cross(wv(w, 0), wv(w, 3)));)
UNIT(u_dop1, 4, 1, RSQ_NONE, put(o, 0, dop1(wf(w, 0), wf(w, 1), wf(w, 2), wf(w, 3)));)
// c. RSQRTSS, from the packed and from the 32-bit LDS table
UNIT(u_rsqrtss_packed, 1, 1, RSQ_PACKED, put(o, 0, rsqrtss_emulated(wf(w, 0), rsq_table(q)));)
UNIT(u_rsqrtss_u32, 1, 1, RSQ_U32, put(o, 0, rsqrtss_emulated(wf(w, 0), rsq_table(q)));)
UNIT(u_rsqrt_ref_packed, 1, 1, RSQ_PACKED, put(o, 0, rsqrt_ref(wf(w, 0), q));)
UNIT(u_rsqrt_ref_u32, 1, 1, RSQ_U32, put(o, 0, rsqrt_ref(wf(w, 0), q));)
// d. shading leaf functions
UNIT(u_fresnel, 3, 1, RSQ_NONE, put(o, 0, fresnel_dielectric(wf(w, 0), wf(w, 1), wf(w, 2)));)
UNIT(u_erfinv, 1, 1, RSQ_NONE, put(o, 0, erfinv(wf(w, 0)));)
UNIT(u_beck11, 3, 2, RSQ_NONE, const P2 s = beckmann_sample11(wf(w, 0), wf(w, 1), wf(w, 2)); put(o, 0, s.x); put(o, 1, s.y);)
// wo, alpha_x, alpha_y, U1, U2: the rho loop's precomputed form, and beckmann_sample11 on the same cosine
UNIT(u_beck11_pre, 7, 4, RSQ_PACKED,
     const Material m = unit_material(wf(w, 3), wf(w, 4), 1.5f);
     const BeckPre  p = beck_pre(m, wv(w, 0), q);
     const P2 s = beckmann_sample11_pre(p, wf(w, 5), wf(w, 6));
     const P2 r = beckmann_sample11(p.st.y, wf(w, 5), wf(w, 6));
     put(o, 0, s.x); put(o, 1, s.y); put(o, 2, r.x); put(o, 3, r.y);)
UNIT(u_uniform_sphere, 2, 3, RSQ_NONE, putv(o, 0, sample_uniform_sphere(wp2(w, 0)));)
UNIT(u_uniform_hemisphere, 2, 3, RSQ_NONE, putv(o, 0, sample_uniform_hemisphere(wp2(w, 0)));)
UNIT(u_concentric_disk, 2, 2, RSQ_NONE, const P2 d = concentric_disk(wp2(w, 0)); put(o, 0, d.x); put(o, 1, d.y);)
UNIT(u_cosine_hemisphere, 2, 3, RSQ_NONE, putv(o, 0, sample_cosine_hemisphere(wp2(w, 0)));)
UNIT(u_onb_of_unit, 3, 9, RSQ_NONE, const Onb b = onb_of_unit(wv(w, 0)); putv(o, 0, b.u); putv(o, 3, b.v); putv(o, 6, b.w);)
UNIT(u_beck_D, 5, 1, RSQ_NONE, put(o, 0, beck_D(unit_material(wf(w, 0), wf(w, 1), 1.5f), wv(w, 2)));)
UNIT(u_beck_lambda, 5, 1, RSQ_NONE, put(o, 0, beck_lambda(unit_material(wf(w, 0), wf(w, 1), 1.5f), wv(w, 2)));)
UNIT(u_beck_pdf, 8, 1, RSQ_NONE, put(o, 0, beck_pdf(unit_material(wf(w, 0), wf(w, 1), 1.5f), wv(w, 2), wv(w, 5)));)
UNIT(u_mf_eval, 9, 3, RSQ_PACKED,
     const rgb c = mf_eval(unit_material(wf(w, 0), wf(w, 1), wf(w, 2)), wv(w, 3), wv(w, 6), q);
     put(o, 0, c.r); put(o, 1, c.g); put(o, 2, c.b);)
UNIT(u_mf_pdf, 8, 1, RSQ_PACKED, put(o, 0, mf_pdf(unit_material(wf(w, 0), wf(w, 1), 1.5f), wv(w, 2), wv(w, 5), q));)
UNIT(u_spherical_phi, 3, 1, RSQ_NONE, put(o, 0, spherical_phi(wv(w, 0)));)
UNIT(u_ray_offset, 6, 1, RSQ_NONE, put(o, 0, ray_offset(wv(w, 0), wv(w, 3)));)
// e. hit tests: flag, then the values of a hit
UNIT(u_tri_hit, 17, 4, RSQ_NONE,
     const float4 q0 = make_float4(wf(w, 0), wf(w, 1), wf(w, 2), 0.0f);
     const float4 q1 = make_float4(wf(w, 3), wf(w, 4), wf(w, 5), 0.0f);
     const float4 q2 = make_float4(wf(w, 6), wf(w, 7), wf(w, 8), 0.0f);
     Ray ray; ray.o = wv(w, 9); ray.d = wv(w, 12);
     float t = 0.0f, b = 0.0f, g = 0.0f;
     const bool hit = tri_hit(q0, q1, q2, ray, wf(w, 15), wf(w, 16), t, b, g);
     o[0] = hit ? 1u : 0u; put(o, 1, hit ? t : 0.0f); put(o, 2, hit ? b : 0.0f); put(o, 3, hit ? g : 0.0f);)
UNIT(u_sphere_t, 20, 2, RSQ_NONE,
     aff m; m.vx = wv(w, 0); m.vy = wv(w, 3); m.vz = wv(w, 6); m.p = wv(w, 9);
     Ray ray; ray.o = wv(w, 12); ray.d = wv(w, 15);
     float t = 0.0f;
     const bool hit = sphere_t(m, ray, wf(w, 18), wf(w, 19), t);
     o[0] = hit ? 1u : 0u; put(o, 1, hit ? t : 0.0f);)
UNIT(u_plane_t, 20, 2, RSQ_NONE,
     aff m; m.vx = wv(w, 0); m.vy = wv(w, 3); m.vz = wv(w, 6); m.p = wv(w, 9);
     Ray ray; ray.o = wv(w, 12); ray.d = wv(w, 15);
     float t = 0.0f;
     const bool hit = plane_t(m, ray, wf(w, 18), wf(w, 19), t);
     o[0] = hit ? 1u : 0u; put(o, 1, hit ? t : 0.0f);)
UNIT(u_box_hit, 14, 1, RSQ_NONE,
     Node nd;
     nd.lo[0] = wf(w, 0); nd.lo[1] = wf(w, 1); nd.lo[2] = wf(w, 2); nd.a = 0u;
     nd.hi[0] = wf(w, 3); nd.hi[1] = wf(w, 4); nd.hi[2] = wf(w, 5); nd.b = 0u;
     Ray ray; ray.o = wv(w, 6); ray.d = wv(w, 9);
     const f3 inv = mk(1.0f / ray.d.x, 1.0f / ray.d.y, 1.0f / ray.d.z); // as every walk forms it
     o[0] = box_hit(nd, ray, inv, wf(w, 12), wf(w, 13)) ? 1u : 0u;)

constexpr int THREADS = 256;

template <class F>
__global__ __launch_bounds__(THREADS) void unit_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, long long n,
                                                       const uint32_t* __restrict__ table, int table_words)
{
    extern __shared__ uint32_t lds[];
    const int tid = threadIdx.x;
    for (int i = tid; i < table_words; i += THREADS) lds[i] = table[i];
    libm_lds_init(tid, blockDim.x);
    __syncthreads();
    const long long row = (long long)blockIdx.x * THREADS + tid;
    if (row >= n) return;
    const Rsq q{ lds };
    uint32_t  w[F::K], o[F::M];
    for (int i = 0; i < F::K; ++i) w[i] = in[row * F::K + i];
    for (int i = 0; i < F::M; ++i) o[i] = 0u;
    F::eval(w, o, q);
    for (int i = 0; i < F::M; ++i) out[row * F::M + i] = o[i];
}

// f. The pixel stream.  Each lane owns a generator in the render kernels' state layout (a wave slot
// of two lane-blocked generation buffers, sp_device.hpp mt_off; the lane's base as
// render_tiles_body forms it) and runs the script of its row: word 0 the seed, word 1 the seeding
// (0 rng_seed, 1 rng_seed_twisted), then STREAM_STEPS steps, each op | prepare << 4 | n << 8.  A
// set prepare bit calls rng_prepare before the step; the scripts set it for whole waves at a time,
// as the kernels call it at wave-synchronous points.  Output: the number of values drawn, then
// every value as next1D forms it, then zeros.
constexpr int STREAM_STEPS = 200, STREAM_K = 2 + STREAM_STEPS, STREAM_M = 2048;
enum { OP_NOP = 0, OP_DRAW = 1, OP_RAW2 = 2, OP_SKIP = 3, OP_RESERVE_DRAW = 4, OP_RESERVE_SKIP = 5 };

__global__ __launch_bounds__(THREADS) void stream_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, long long n,
                                                         uint64_t* mt_state)
{
    const int tid = threadIdx.x;
    libm_lds_init(tid, blockDim.x);
    __syncthreads();
    const long long row = (long long)blockIdx.x * THREADS + tid;
    if (row >= n) return; // n is a multiple of 64: whole waves leave
    const int    lane  = tid & 63;
    const size_t gwave = (size_t)blockIdx.x * (THREADS / 64) + (size_t)(tid >> 6);
    Rng          rng;
    rng.base = mt_state + gwave * (2 * (size_t)MT_GEN_WORDS) + (size_t)lane * MT_BLK;
    const uint32_t* w = in + row * STREAM_K;
    uint32_t*       o = out + row * STREAM_M;
    if (w[1]) rng_seed_twisted(rng, w[0]);
    else rng_seed(rng, w[0]);
    int  cnt  = 0;
    auto emit = [&](float f) {
        if (cnt < STREAM_M - 1) o[1 + cnt] = __float_as_uint(f);
        ++cnt;
    };
    for (int s = 0; s < STREAM_STEPS; ++s) {
        const uint32_t step = w[2 + s];
        const int      op = (int)(step & 15u), k = (int)(step >> 8);
        if (step & 16u) rng_prepare(rng);
        if (op == OP_DRAW) {
            for (int i = 0; i < k; ++i) emit(next1D(rng));
        } else if (op == OP_RAW2) {
            uint64_t a, b;
            rng_raw2(rng, a, b);
            emit(canonical_from_u64(a));
            emit(canonical_from_u64(b));
        } else if (op == OP_SKIP) {
            rng_skip(rng, k);
        } else if (op == OP_RESERVE_DRAW) {
            rng_reserve(rng, k);
            for (int i = 0; i < k; ++i) emit(next1D<true>(rng));
        } else if (op == OP_RESERVE_SKIP) {
            rng_reserve(rng, k);
            rng_skip_reserved(rng, k);
        }
    }
    o[0] = (uint32_t)cnt;
    for (int i = 1 + (cnt < STREAM_M - 1 ? cnt : STREAM_M - 1); i < STREAM_M; ++i) o[i] = 0u;
}

// g. The stream-fed layer: what takes a material or light record and a pixel stream and draws
// from it.  A row that draws starts with seed, skip; the lane owns a generator as in stream_kernel,
// seeds it (odd rows rng_seed_twisted, even rows rng_seed), calls rng_skip(skip) and evaluates.  Its
// last two output words are the rng.draws delta of the evaluation and one further next1D.
// Material record, 26 words: kind, albedo, microfacet_r, alpha_x, alpha_y, ior, sample_visible_area,
// coat_ior, coat_color, then a clearcoat's base record (kind .. sample_visible_area, 11 words); the
// lane builds a two-entry material table from it (entry 0 the record, entry 1 its base).
// Light record, 37 words: kind, radiance, object_to_world, world_to_object, normal_to_world.
constexpr int ROW_MAT = 26, ROW_LIGHT = 37;
__device__ __forceinline__ Material row_record(const uint32_t* w)
{
    Material m;
    m.kind = (int32_t)w[0]; m.base = -1;
    m.lambert_albedo = mkc(wf(w, 1), wf(w, 2), wf(w, 3));
    m.microfacet_r   = mkc(wf(w, 4), wf(w, 5), wf(w, 6));
    m.alpha_x = wf(w, 7); m.alpha_y = wf(w, 8); m.microfacet_ior = wf(w, 9);
    m.sample_visible_area = (int32_t)w[10];
    m.coat_ior   = 0.0f;
    m.coat_color = mkc(0, 0, 0);
    return m;
}
struct RowScene {
    Material mats[2];
    Scene    sc;
};
__device__ __forceinline__ void row_scene(const uint32_t* w, RowScene& s)
{
    s.mats[0]            = row_record(w);
    s.mats[1]            = row_record(w + 15);
    s.mats[0].coat_ior   = wf(w, 11);
    s.mats[0].coat_color = mkc(wf(w, 12), wf(w, 13), wf(w, 14));
    if (s.mats[0].kind == SP_MAT_CLEARCOAT) s.mats[0].base = 1;
    s.sc           = Scene{};
    s.sc.materials = s.mats;
}
__device__ __forceinline__ aff row_aff(const uint32_t* w) { aff m; m.vx = wv(w, 0); m.vy = wv(w, 3); m.vz = wv(w, 6); m.p = wv(w, 9); return m; }
__device__ __forceinline__ Light row_light(const uint32_t* w)
{
    Light l;
    l.kind = (int32_t)w[0]; l.image = -1;
    l.radiance = mkc(wf(w, 1), wf(w, 2), wf(w, 3));
    l.o2w = row_aff(w + 4);
    l.w2o = row_aff(w + 16);
    l.nrm.vx = wv(w, 28); l.nrm.vy = wv(w, 31); l.nrm.vz = wv(w, 34);
    return l;
}
__device__ __forceinline__ void put_sample(uint32_t* o, const MSample& s)
{
    put(o, 0, s.color.r); put(o, 1, s.color.g); put(o, 2, s.color.b);
    putv(o, 3, s.dir); put(o, 6, s.pdf); o[7] = (uint32_t)s.props;
}

// w: the whole row (seed, skip, material record, directions); v: its directions
#define DRAW_UNIT(NAME, KK, MM, ...)                                                                                   \
    struct NAME {                                                                                                      \
        static constexpr int K = KK, M = MM, TABLE = RSQ_PACKED;                                                       \
        static __device__ __forceinline__ void eval(const uint32_t* w, uint32_t* o, const Rsq& q, Rng& rng)            \
        {                                                                                                              \
            const uint32_t* v = w + 2 + ROW_MAT;                                                                       \
            __VA_ARGS__                                                                                                \
        }                                                                                                              \
    };

// the estimate in the instantiation this option set's kernels make for a lane's own estimate
DRAW_UNIT(u_rho16, 31, 5, const rgb c = mf_rho16(row_record(w + 2), wv(v, 0), rng, q); put(o, 0, c.r); put(o, 1, c.g); put(o, 2, c.b);)
DRAW_UNIT(u_glossy_weights, 31, 4, float wt[2]; glossy_weights(row_record(w + 2), wv(v, 0), rng, q, wt); put(o, 0, wt[0]); put(o, 1, wt[1]);)
DRAW_UNIT(u_mf_sample, 31, 10, put_sample(o, mf_sample(row_record(w + 2), wv(v, 0), rng, q));)
DRAW_UNIT(u_mf_sample_pre, 31, 10,
          const Material m = row_record(w + 2);
          const BeckPre  p = beck_pre(m, wv(v, 0), q);
          put_sample(o, mf_sample_pre(m, p, wv(v, 0), rng, q));)
// world form: n, wo, then wi
DRAW_UNIT(u_material_sample, 34, 10, RowScene s; row_scene(w + 2, s); put_sample(o, material_sample(s.sc, 0, wv(v, 3), wv(v, 0), rng, q));)
DRAW_UNIT(u_material_eval, 37, 5,
          RowScene s; row_scene(w + 2, s);
          const rgb c = material_eval(s.sc, 0, wv(v, 3), wv(v, 6), wv(v, 0), rng, q);
          put(o, 0, c.r); put(o, 1, c.g); put(o, 2, c.b);)
DRAW_UNIT(u_material_pdf, 37, 3, RowScene s; row_scene(w + 2, s); put(o, 0, material_pdf(s.sc, 0, wv(v, 3), wv(v, 6), wv(v, 0), rng, q));)
#if SP_SERVE_RHO
// The served forms (IterativeRRNEE): the estimate in the instantiation served estimates use, and
// served_weights reading the lane's own words the way serve_rho reads an owner's: the owner
// reserves, the position is taken as (buffer, index), and the owner skips the words afterwards.
DRAW_UNIT(u_rho16_served, 31, 5,
          const rgb c = mf_rho16<(SP_SERVED_PAIR != 0), (SP_SERVED_ALIGNED != 0), (SP_SERVED_TOUCH != 0)>(row_record(w + 2), wv(v, 0), rng, q);
          put(o, 0, c.r); put(o, 1, c.g); put(o, 2, c.b);)
DRAW_UNIT(u_weights_served, 31, 4,
          const f3  wo = wv(v, 0);
          const int dc = (wo.y == 0.0f) ? 0 : 32;
          rng_reserve(rng, dc);
          int cur = rng.cur, idx = rng.idx;
          if (idx >= MT_N) { cur ^= 1; idx -= MT_N; }
          float wt[2];
          served_weights(row_record(w + 2), wo, rng.base, cur, idx, q, wt);
          rng_skip_reserved(rng, dc);
          put(o, 0, wt[0]); put(o, 1, wt[1]);)
#endif
// lights: record, observer, then its normal and u (light_sample) or wi (light_pdf)
UNIT(u_sphere_pdf, 40, 1, RSQ_NONE, put(o, 0, sphere_pdf(row_light(w), wv(w, ROW_LIGHT)));)
UNIT(u_light_sample, 45, 9, RSQ_PACKED,
     const Scene   sc{};
     const LSample s = light_sample(sc, row_light(w), wv(w, ROW_LIGHT), wv(w, ROW_LIGHT + 3), wp2(w, ROW_LIGHT + 6), q);
     put(o, 0, s.L.r); put(o, 1, s.L.g); put(o, 2, s.L.b); put(o, 3, s.pdf); putv(o, 4, s.ray.d); put(o, 7, s.tmin); put(o, 8, s.tmax);)
UNIT(u_light_pdf, 43, 1, RSQ_NONE, const Scene sc{}; put(o, 0, light_pdf(sc, row_light(w), wv(w, ROW_LIGHT), wv(w, ROW_LIGHT + 3)));)

template <class F>
__global__ __launch_bounds__(THREADS) void draw_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, long long n,
                                                       const uint32_t* __restrict__ table, int table_words, uint64_t* mt_state, void*)
{
    extern __shared__ uint32_t lds[];
    const int tid = threadIdx.x;
    for (int i = tid; i < table_words; i += THREADS) lds[i] = table[i];
    libm_lds_init(tid, blockDim.x);
    __syncthreads();
    const long long row = (long long)blockIdx.x * THREADS + tid;
    if (row >= n) return;
    const Rsq    q{ lds };
    const int    lane  = tid & 63;
    const size_t gwave = (size_t)blockIdx.x * (THREADS / 64) + (size_t)(tid >> 6);
    Rng          rng;
    rng.base = mt_state + gwave * (2 * (size_t)MT_GEN_WORDS) + (size_t)lane * MT_BLK;
    uint32_t w[F::K], o[F::M];
    for (int i = 0; i < F::K; ++i) w[i] = in[row * F::K + i];
    for (int i = 0; i < F::M; ++i) o[i] = 0u;
    if (row & 1) rng_seed_twisted(rng, w[0]);
    else rng_seed(rng, w[0]);
    rng_skip(rng, (int)w[1]);
    const uint32_t before = rng.draws;
    F::eval(w, o, q, rng);
    o[F::M - 2] = rng.draws - before;
    put(o, F::M - 1, next1D(rng));
    for (int i = 0; i < F::M; ++i) out[row * F::M + i] = o[i];
}

#if SP_SERVE_RHO
// serve_rho (IterativeRRNEE).  64 consecutive rows are one wave; each row is one lane's request: seed,
// skip, a material record, n, wo, flags (1: wants the three estimates of a light's eval / pdf / sample,
// 2: wants the estimate of the bounce's own deferred Material::sample, 4: leaves before the call, as
// the lanes of a clipped border tile never enter).  The lane follows integrate_rrnee: a bounce that
// defers its sample reserves 140 words, draws a clearcoat's Fresnel pick (a specular pick undoes the
// draw and wants nothing), notes srv_posA / srv_pwA and skips the estimate and the sample's three
// words; the light's sample draws two; every lane that is here calls serve_rho (the material table
// is one for all lanes, built by serve_materials: a dealt lane reads the owner's record by index); the deferred
// sample's site takes its weights from a copy of the stream at the bounce's position, then the
// eval, pdf and sample sites of the light take theirs, all through glossy_weights.
// Output: whether the bounce's site was served, its weights, the words it consumed (the coat's
// draw and the estimate); the weights of the eval, pdf and sample sites and the words they consumed;
// one further next1D.
constexpr int SERVE_K = 2 + ROW_MAT + 7, SERVE_M = 12;
// the scene's material table, as the lanes of a wave share it: row r's record at 2r, its base record at 2r + 1
__global__ __launch_bounds__(THREADS) void serve_materials(const uint32_t* __restrict__ in, long long n, Material* mats)
{
    const long long row = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (row >= n) return;
    uint32_t w[ROW_MAT];
    for (int i = 0; i < ROW_MAT; ++i) w[i] = in[row * SERVE_K + 2 + i];
    RowScene s;
    row_scene(w, s);
    if (s.mats[0].base >= 0) s.mats[0].base = (int32_t)(2 * row + 1);
    mats[2 * row]     = s.mats[0];
    mats[2 * row + 1] = s.mats[1];
}
__global__ __launch_bounds__(THREADS) void serve_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, long long n,
                                                        const uint32_t* __restrict__ table, int table_words, uint64_t* mt_state,
                                                        void* materials)
{
    extern __shared__ uint32_t lds[];
    const int tid = threadIdx.x;
    for (int i = tid; i < table_words; i += THREADS) lds[i] = table[i];
    libm_lds_init(tid, blockDim.x);
    __syncthreads();
    const long long row = (long long)blockIdx.x * THREADS + tid;
    if (row >= n) return; // n is a multiple of 64: whole waves leave
    const Rsq    q{ lds };
    const int    lane  = tid & 63;
    const size_t gwave = (size_t)blockIdx.x * (THREADS / 64) + (size_t)(tid >> 6);
    uint32_t     w[SERVE_K], o[SERVE_M];
    for (int i = 0; i < SERVE_K; ++i) w[i] = in[row * SERVE_K + i];
    for (int i = 0; i < SERVE_M; ++i) o[i] = 0u;
    const uint32_t flags = w[SERVE_K - 1];
    if (flags & 4u) { // never enters: not one of the lanes the requests are dealt to
        for (int i = 0; i < SERVE_M; ++i) out[row * SERVE_M + i] = 0u;
        return;
    }
    Rng rng;
    rng.base = mt_state + gwave * (2 * (size_t)MT_GEN_WORDS) + (size_t)lane * MT_BLK;
    if (row & 1) rng_seed_twisted(rng, w[0]);
    else rng_seed(rng, w[0]);
    rng_skip(rng, (int)w[1]);
    Scene sc{};
    sc.materials = static_cast<const Material*>(materials);
    const int       mid = (int)(2 * row);
    const uint32_t* v   = w + 2 + ROW_MAT;
    const f3        nn = wv(v, 0), wo = wv(v, 3);
    const Material& mm   = sc.materials[mid];
    const bool      coat = mm.kind == SP_MAT_CLEARCOAT;
    const Material& base = sc.materials[coat ? mm.base : mid];
    const f3        wl   = to_onb(onb_from_v(nn, q), wo);
    Ctx  c{ sc, rng, q, Stack{ nullptr, lane, 0 }, 0u, 0u };
    const bool want = (flags & 1u) != 0;
    bool       pend = false;
    Rng        snap = rng;
    if (flags & 2u) { // integrate_rrnee's deferred Material::sample
        rng_reserve(rng, 140);
        snap      = rng;
        bool spec = false;
        if (coat) spec = next1D(rng) < fresnel_dielectric(wl.y, 1.0f, mm.coat_ior);
        if (spec) {
            rng = snap;
        } else {
            pend         = true;
            rng.srv_dc   = (wl.y == 0.0f) ? 0u : 32u;
            rng.srv_posA = rng.draws;
            rng.srv_pwA  = ((uint32_t)rng.cur << 16) | (uint32_t)rng.idx;
            rng_skip_reserved(rng, (int)rng.srv_dc + 3);
        }
    }
    (void)next2D(rng); // the light's sample
    serve_rho(c, want, pend, mid, nn, wo);
    float wt[2];
    if (pend) {
        Rng ra      = snap;
        ra.srv_on   = 1;
        ra.srv_A    = true;
        ra.srv_B    = false;
        ra.srv_posA = rng.srv_posA;
        ra.srv_dc   = rng.srv_dc;
        if (coat) (void)next1D(ra); // material_sample_local's Fresnel pick, drawn again
        glossy_weights(base, wl, ra, q, wt);
        rng.srv_A = false;
        o[0] = 1u; put(o, 1, wt[0]); put(o, 2, wt[1]); o[3] = ra.draws - snap.draws;
    }
    const uint32_t before = rng.draws;
    if (want) { // Material::eval, Material::pdf, Material::sample (its coat pick first) of estimate_direct_mis
        glossy_weights(base, wl, rng, q, wt);
        put(o, 4, wt[0]); put(o, 5, wt[1]);
        glossy_weights(base, wl, rng, q, wt);
        put(o, 6, wt[0]); put(o, 7, wt[1]);
        if (coat) (void)next1D(rng);
        glossy_weights(base, wl, rng, q, wt);
        put(o, 8, wt[0]); put(o, 9, wt[1]);
    }
    rng.srv_on = 0;
    rng.srv_B  = false;
    o[10] = rng.draws - before;
    put(o, 11, next1D(rng));
    for (int i = 0; i < SERVE_M; ++i) out[row * SERVE_M + i] = o[i];
}
#endif

#define HIP_OK(expr)                                                                                                   \
    do {                                                                                                               \
        const hipError_t e_ = (expr);                                                                                  \
        if (e_ != hipSuccess) {                                                                                        \
            std::fprintf(stderr, "device_units: %s: %s\n", #expr, hipGetErrorString(e_));                              \
            std::exit(3); /* nothing further is launched after a HIP error */                                          \
        }                                                                                                              \
    } while (0)

template <class F>
float launch(const uint32_t* in, uint32_t* out, long long n, const uint32_t* table, int table_words)
{
    const size_t lds_bytes = (size_t)(table_words > 0 ? table_words : 8) * sizeof(uint32_t);
    if (lds_bytes > 32768)
        HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(&unit_kernel<F>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lds_bytes));
    hipFuncAttributes attr; // loads the code object, so the events below time the kernel alone
    HIP_OK(hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(&unit_kernel<F>)));
    hipEvent_t t0, t1;
    HIP_OK(hipEventCreate(&t0));
    HIP_OK(hipEventCreate(&t1));
    const unsigned blocks = (unsigned)((n + THREADS - 1) / THREADS);
    HIP_OK(hipEventRecord(t0));
    unit_kernel<F><<<blocks, THREADS, lds_bytes>>>(in, out, n, table, table_words);
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(t1));
    HIP_OK(hipEventSynchronize(t1));
    HIP_OK(hipDeviceSynchronize());
    float ms = 0.0f;
    HIP_OK(hipEventElapsedTime(&ms, t0, t1));
    return ms;
}

float launch_stream(const uint32_t* in, uint32_t* out, long long n, const uint32_t*, int)
{
    if (n % 64 != 0) {
        std::fprintf(stderr, "device_units: stream needs whole waves, %lld rows are no multiple of 64\n", n);
        std::exit(2);
    }
    const unsigned blocks = (unsigned)((n + THREADS - 1) / THREADS);
    // one wave slot (two generation buffers of 64 lane-blocked streams) per wave of the grid
    const size_t state_words = (size_t)blocks * (THREADS / 64) * 2 * (size_t)MT_GEN_WORDS;
    uint64_t*    state       = nullptr;
    HIP_OK(hipMalloc(&state, state_words * sizeof(uint64_t)));
    HIP_OK(hipMemset(state, 0, state_words * sizeof(uint64_t)));
    hipFuncAttributes attr;
    HIP_OK(hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(&stream_kernel)));
    hipEvent_t t0, t1;
    HIP_OK(hipEventCreate(&t0));
    HIP_OK(hipEventCreate(&t1));
    HIP_OK(hipEventRecord(t0));
    stream_kernel<<<blocks, THREADS>>>(in, out, n, state);
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(t1));
    HIP_OK(hipEventSynchronize(t1));
    HIP_OK(hipDeviceSynchronize());
    float ms = 0.0f;
    HIP_OK(hipEventElapsedTime(&ms, t0, t1));
    HIP_OK(hipFree(state));
    return ms;
}

// h. The image environment light, against a small image given as one more file argument: w, h,
// max_radiance, light_to_world, world_to_light (9 words each), then w * h * 3 pixel words.  The
// tables are the ones the upload's own host builder makes (sp_envmap.cpp build_env_map), copied to
// the device as the upload copies them; the _replay names run the same functions without the guide
// tables (the replayed upper_bound of dist_offset).
#define ENV_UNIT(NAME, KK, MM, ...)                                                                                    \
    struct NAME {                                                                                                      \
        static constexpr int K = KK, M = MM, TABLE = RSQ_PACKED;                                                       \
        static __device__ __forceinline__ void eval(const uint32_t* w, uint32_t* o, const Rsq& q, const EnvMap& e) { __VA_ARGS__ } \
    };
ENV_UNIT(u_env_sample, 2, 7, const EnvSample s = env_sample(e, wp2(w, 0));
         put(o, 0, s.L.r); put(o, 1, s.L.g); put(o, 2, s.L.b); put(o, 3, s.pdf); putv(o, 4, s.wi);)
ENV_UNIT(u_env_pdf, 3, 1, put(o, 0, env_pdf(e, wv(w, 0)));)
ENV_UNIT(u_env_radiance, 3, 3, const rgb c = env_radiance(e, wv(w, 0), q); put(o, 0, c.r); put(o, 1, c.g); put(o, 2, c.b);)

template <class F>
__global__ __launch_bounds__(THREADS) void env_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, long long n,
                                                      const uint32_t* __restrict__ table, int table_words, const EnvMap e)
{
    extern __shared__ uint32_t lds[];
    const int tid = threadIdx.x;
    for (int i = tid; i < table_words; i += THREADS) lds[i] = table[i];
    libm_lds_init(tid, blockDim.x);
    __syncthreads();
    const long long row = (long long)blockIdx.x * THREADS + tid;
    if (row >= n) return;
    const Rsq q{ lds };
    uint32_t  w[F::K], o[F::M];
    for (int i = 0; i < F::K; ++i) w[i] = in[row * F::K + i];
    for (int i = 0; i < F::M; ++i) o[i] = 0u;
    F::eval(w, o, q, e);
    for (int i = 0; i < F::M; ++i) out[row * F::M + i] = o[i];
}

EnvMap g_env;         // device tables of the image argument (main)
bool   g_env_set = false;

template <class F, bool REPLAY>
float launch_env(const uint32_t* in, uint32_t* out, long long n, const uint32_t* table, int table_words)
{
    if (!g_env_set) {
        std::fprintf(stderr, "device_units: this function needs the image file\n");
        std::exit(2);
    }
    EnvMap e = g_env;
    if (REPLAY) e.cond_guide = e.marg_guide = nullptr;
    const size_t lds_bytes = (size_t)(table_words > 0 ? table_words : 8) * sizeof(uint32_t);
    if (lds_bytes > 32768)
        HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(&env_kernel<F>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lds_bytes));
    hipFuncAttributes attr;
    HIP_OK(hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(&env_kernel<F>)));
    hipEvent_t t0, t1;
    HIP_OK(hipEventCreate(&t0));
    HIP_OK(hipEventCreate(&t1));
    const unsigned blocks = (unsigned)((n + THREADS - 1) / THREADS);
    HIP_OK(hipEventRecord(t0));
    env_kernel<F><<<blocks, THREADS, lds_bytes>>>(in, out, n, table, table_words, e);
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(t1));
    HIP_OK(hipEventSynchronize(t1));
    HIP_OK(hipDeviceSynchronize());
    float ms = 0.0f;
    HIP_OK(hipEventElapsedTime(&ms, t0, t1));
    return ms;
}

template <class T>
const T* to_device(const std::vector<T>& v)
{
    T* d = nullptr;
    HIP_OK(hipMalloc(&d, (v.empty() ? 1 : v.size()) * sizeof(T)));
    if (!v.empty()) HIP_OK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return d;
}
lin words_lin(const uint32_t* w)
{
    float f[9];
    std::memcpy(f, w, sizeof f);
    lin l;
    l.vx = mk(f[0], f[1], f[2]); l.vy = mk(f[3], f[4], f[5]); l.vz = mk(f[6], f[7], f[8]);
    return l;
}
// the image file -> the device's EnvMap (freed with the process)
bool set_env(const std::vector<uint32_t>& f)
{
    if (f.size() < 21) return false;
    sph::EnvImage img;
    img.width = (int)f[0]; img.height = (int)f[1];
    if (img.width < 1 || img.height < 1 || img.width > 4096 || img.height > 4096) return false;
    if (f.size() != 21 + (size_t)img.width * (size_t)img.height * 3) return false;
    std::memcpy(&img.max_radiance, &f[2], 4);
    img.light_to_world = words_lin(&f[3]);
    img.world_to_light = words_lin(&f[12]);
    img.pixels.resize(f.size() - 21);
    std::memcpy(img.pixels.data(), &f[21], img.pixels.size() * 4);
    const sph::EnvMap m = sph::build_env_map(img);
    if (!m.guided) return false; // the rows hold no NaN texel: both lookup forms exist
    std::vector<float4> rad((size_t)m.w * (size_t)m.h);
    for (size_t p = 0; p < rad.size(); ++p) rad[p] = make_float4(m.radiance[p * 3], m.radiance[p * 3 + 1], m.radiance[p * 3 + 2], 0.0f);
    g_env.l2w = img.light_to_world; g_env.w2l = img.world_to_light;
    g_env.w = m.w; g_env.h = m.h; g_env.nu = m.nu; g_env.nv = m.nv;
    g_env.radiance  = to_device(rad);
    g_env.cond_func = to_device(m.cond_func);
    g_env.cond_cdf  = to_device(m.cond_cdf);
    g_env.cond_int  = to_device(m.cond_int);
    g_env.marg_func = to_device(m.marg_func);
    g_env.marg_cdf  = to_device(m.marg_cdf);
    g_env.marg_int  = m.marg_int;
    g_env.cond_guide = to_device(m.cond_guide);
    g_env.marg_guide = to_device(m.marg_guide);
    g_env.cond_bits = m.cond_bits; g_env.marg_bits = m.marg_bits;
    g_env_set = true;
    return true;
}

// a kernel whose lanes own generators: one wave slot of state per wave of the grid
template <class Kern>
float launch_with_state(Kern kern, const uint32_t* in, uint32_t* out, long long n, const uint32_t* table, int table_words,
                        void* extra = nullptr)
{
    const size_t lds_bytes = (size_t)(table_words > 0 ? table_words : 8) * sizeof(uint32_t);
    if (lds_bytes > 32768)
        HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    const unsigned blocks = (unsigned)((n + THREADS - 1) / THREADS);
    // one wave slot (two generation buffers of 64 lane-blocked streams) per wave of the grid
    const size_t state_words = (size_t)blocks * (THREADS / 64) * 2 * (size_t)MT_GEN_WORDS;
    uint64_t*    state       = nullptr;
    HIP_OK(hipMalloc(&state, state_words * sizeof(uint64_t)));
    HIP_OK(hipMemset(state, 0, state_words * sizeof(uint64_t)));
    hipFuncAttributes attr;
    HIP_OK(hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(kern)));
    hipEvent_t t0, t1;
    HIP_OK(hipEventCreate(&t0));
    HIP_OK(hipEventCreate(&t1));
    HIP_OK(hipEventRecord(t0));
    kern<<<blocks, THREADS, lds_bytes>>>(in, out, n, table, table_words, state, extra);
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(t1));
    HIP_OK(hipEventSynchronize(t1));
    HIP_OK(hipDeviceSynchronize());
    float ms = 0.0f;
    HIP_OK(hipEventElapsedTime(&ms, t0, t1));
    HIP_OK(hipFree(state));
    return ms;
}
template <class F>
float launch_draw(const uint32_t* in, uint32_t* out, long long n, const uint32_t* table, int table_words)
{
    return launch_with_state(&draw_kernel<F>, in, out, n, table, table_words);
}
#if SP_SERVE_RHO
float launch_serve(const uint32_t* in, uint32_t* out, long long n, const uint32_t* table, int table_words)
{
    if (n % 64 != 0) {
        std::fprintf(stderr, "device_units: serve_rho needs whole waves, %lld rows are no multiple of 64\n", n);
        std::exit(2);
    }
    Material* mats = nullptr;
    HIP_OK(hipMalloc(&mats, (size_t)n * 2 * sizeof(Material)));
    serve_materials<<<(unsigned)((n + THREADS - 1) / THREADS), THREADS>>>(in, n, mats);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    const float ms = launch_with_state(&serve_kernel, in, out, n, table, table_words, mats);
    HIP_OK(hipFree(mats));
    return ms;
}
#endif

struct Function {
    const char* name;
    int         k, m, table;
    float (*run)(const uint32_t*, uint32_t*, long long, const uint32_t*, int);
};
#define FN(NAME) { #NAME, u_##NAME::K, u_##NAME::M, u_##NAME::TABLE, &launch<u_##NAME> }
#define ENV(NAME) { #NAME, u_##NAME::K, u_##NAME::M, u_##NAME::TABLE, &launch_env<u_##NAME, false> },                                \
                  { #NAME "_replay", u_##NAME::K, u_##NAME::M, u_##NAME::TABLE, &launch_env<u_##NAME, true> }
#define DRAW(NAME) { #NAME, u_##NAME::K, u_##NAME::M, u_##NAME::TABLE, &launch_draw<u_##NAME> }
const Function FUNCTIONS[] = {
    FN(expf), FN(logf), FN(sinf), FN(cosf), FN(erff), FN(acosf), FN(atanf), FN(fmod1), FN(roundf), FN(sincosf),
    FN(sincosf_bounded), FN(powf), FN(atan2f), FN(powf_unit), FN(div), FN(sqrt), FN(fma), FN(muladd), FN(sqrt_unit),
    FN(dot), FN(cross), FN(dop1), FN(rsqrtss_packed), FN(rsqrtss_u32), FN(rsqrt_ref_packed), FN(rsqrt_ref_u32),
    FN(fresnel), FN(erfinv), FN(beck11), FN(beck11_pre), FN(uniform_sphere), FN(uniform_hemisphere),
    FN(concentric_disk), FN(cosine_hemisphere), FN(onb_of_unit), FN(beck_D), FN(beck_lambda), FN(beck_pdf),
    FN(mf_eval), FN(mf_pdf), FN(spherical_phi), FN(ray_offset), FN(tri_hit), FN(sphere_t), FN(plane_t), FN(box_hit),
    { "stream", STREAM_K, STREAM_M, RSQ_NONE, &launch_stream },
    DRAW(rho16), DRAW(glossy_weights), DRAW(mf_sample), DRAW(mf_sample_pre), DRAW(material_sample), DRAW(material_eval),
    DRAW(material_pdf),
#if SP_SERVE_RHO
    DRAW(rho16_served), DRAW(weights_served),
    { "serve_rho", SERVE_K, SERVE_M, RSQ_PACKED, &launch_serve },
#endif
    FN(sphere_pdf), FN(light_sample), FN(light_pdf),
    ENV(env_sample), ENV(env_pdf), ENV(env_radiance),
};

bool read_words(const char* path, std::vector<uint32_t>& words)
{
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    if (bytes < 0 || bytes % 4 != 0) { std::fclose(f); return false; }
    words.resize((size_t)bytes / 4);
    const size_t got = words.empty() ? 0 : std::fread(words.data(), 4, words.size(), f);
    std::fclose(f);
    return got == words.size();
}

int fail(const std::string& msg)
{
    std::fprintf(stderr, "device_units: %s\n", msg.c_str());
    return 2;
}

} // namespace

int main(int argc, char** argv)
{
    if (argc < 4 || argc > 6) return fail("usage: device_units <function> <in.bin> <out.bin> [rsqrt_table.bin [image.bin]]");
    const Function* fn = nullptr;
    for (const Function& f : FUNCTIONS)
        if (std::strcmp(f.name, argv[1]) == 0) fn = &f;
    if (!fn) return fail(std::string("unknown function ") + argv[1]);

    std::vector<uint32_t> in;
    if (!read_words(argv[2], in)) return fail(std::string("cannot read whole words from ") + argv[2]);
    if (in.empty() || in.size() % (size_t)fn->k != 0)
        return fail(std::string(argv[2]) + ": short file, " + std::to_string(in.size()) + " words are no rows of " + std::to_string(fn->k));
    const long long n = (long long)(in.size() / (size_t)fn->k);
    if (n > (1ll << 26)) return fail("more than 2^26 rows");

    std::vector<uint32_t> table; // device form: header + entries
    if (fn->table != RSQ_NONE) {
        if (argc < 5) return fail(std::string(fn->name) + " needs the RSQRTSS table file");
        std::vector<uint32_t> t;
        if (!read_words(argv[4], t) || t.size() < 3 || t[0] < 1u || t[0] > 13u || t.size() != 3 + ((size_t)2 << t[0]))
            return fail(std::string(argv[4]) + ": not bits, zero_result, denorm_result and 2 << bits entries");
        table = rsqrt_device_words(t.data() + 3, t.size() - 3, (int32_t)t[0], t[1], t[2], fn->table == RSQ_PACKED);
        if (fn->table == RSQ_PACKED && table[3] == 0u) return fail("this host's RSQRTSS table does not pack to 16-bit entries");
    }

    if (argc == 6) {
        std::vector<uint32_t> img;
        if (!read_words(argv[5], img) || !set_env(img))
            return fail(std::string(argv[5]) + ": not w, h, max_radiance, two 3x3 transforms and w * h * 3 ordered pixel words");
    }

    uint32_t *d_in = nullptr, *d_out = nullptr, *d_table = nullptr;
    const size_t out_words = (size_t)n * (size_t)fn->m;
    HIP_OK(hipMalloc(&d_in, in.size() * 4));
    HIP_OK(hipMalloc(&d_out, out_words * 4));
    HIP_OK(hipMemcpy(d_in, in.data(), in.size() * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(d_out, 0xff, out_words * 4));
    if (!table.empty()) {
        HIP_OK(hipMalloc(&d_table, table.size() * 4));
        HIP_OK(hipMemcpy(d_table, table.data(), table.size() * 4, hipMemcpyHostToDevice));
    }
    const float ms = fn->run(d_in, d_out, n, d_table, (int)table.size());
    std::vector<uint32_t> out(out_words);
    HIP_OK(hipMemcpy(out.data(), d_out, out_words * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipFree(d_in));
    HIP_OK(hipFree(d_out));
    if (d_table) HIP_OK(hipFree(d_table));

    FILE* f = std::fopen(argv[3], "wb");
    if (!f || std::fwrite(out.data(), 4, out.size(), f) != out.size() || std::fclose(f) != 0)
        return fail(std::string("cannot write ") + argv[3]);
    std::printf("%s %lld %.3f\n", fn->name, n, ms);
    return 0;
}
