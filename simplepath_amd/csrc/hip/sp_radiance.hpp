// sp_radiance.hpp -- radiance queries (sp_scene_radiance_rays): the reference's
// Integrator::integrate (Integrators/Integrator.h:37) along rays the caller brings, each with a
// sampler seed of its own.  The fifth family of the persistent megakernel, with a body of its own:
// it shares integrate<INTEG>(c, ray) and everything below it with render_tiles_body (sp_mega.hpp),
// and nothing of the tile, pixel or camera code above it.  Instantiated per integrator in
// sp_radiance*.hip, each with the sampler options of the integrator's one-shot kernel.
#pragma once
#include "sp_mega.hpp"

namespace spd {
inline namespace SPD_LAYOUT_NS {

__device__ __forceinline__ bool radiance_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// Queue item `item` is records [64 item, 64 item + 64): lane l owns record 64 item + l for all its
// samples, as a lane owns a pixel in render_tiles_body.  A record is the sampler seed and the ray,
// two 16-byte loads per lane; the lane seeds the record's mt19937_64 (get_integrator_sampler,
// main.cpp:73, with the caller's seed), calls the integrator spp times with the stream running on,
// sums in call order, divides and stores three floats (main.cpp:94-102 for one pixel).  A record
// past num_rays, or one whose ray no integrator makes (a component that is not finite, a zero
// direction), sits the item out under divergence as a pixel outside the image does in a clipped
// tile: it seeds nothing, walks nothing and counts nothing; the latter's radiance is +0.
template <int INTEG>
__device__ __forceinline__ void radiance_rays_body(const Scene& sc, const RenderArgs& args, const RadianceArgs& ra)
{
    static_assert(INTEG != SP_INTEGRATOR_MANDELBROT, "Mandelbrot has no ray");
    extern __shared__ uint32_t lds[];
    const int tid  = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    // render_tiles_body's prologue: the RSQRTSS table and the libm tables into LDS, then this
    // wave's traversal stack and generator rows
    const int rs_words = rsqrt_words(sc);
    for (int i = tid; i < rs_words; i += 64 * WAVES_PER_BLOCK) lds[i] = sc.rsqrt_entries[i];
    libm_lds_init(tid, 64 * WAVES_PER_BLOCK);
    __syncthreads();
    Rsq   q{ lds };
    Stack st{ lds + rs_words + wave * sc.stack_words * 64, lane, sc.stack_depth };

    const size_t gwave = (size_t)blockIdx.x * WAVES_PER_BLOCK + wave;
    Rng          rng;
    rng.base = args.mt_state + gwave * (2 * (size_t)MT_GEN_WORDS) + (size_t)lane * MT_BLK;

    uint32_t rays_total = 0, shadow_total = 0, samples_total = 0, draws_total = 0;
    while (true) {
        int grabbed = 0;
        if (lane == 0) grabbed = atomicAdd(args.tile_counter, 1);
        // unsigned: a queue head that the waves' last grabs carried past INT32_MAX ends the loop
        const int64_t item = (int64_t)(uint32_t)__shfl(grabbed, 0, 64);
        if (item >= args.num_tiles) break;
        const int64_t i      = item * 64 + lane;
        const bool    listed = i < ra.num_rays;
        float4        r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = r0; // {o, seed}, {d, reserved}
        if (listed) {
            const float4* p = reinterpret_cast<const float4*>(ra.rays + i);
            r0              = p[0];
            r1              = p[1];
        }
        const bool finite = radiance_finite(r0.x) && radiance_finite(r0.y) && radiance_finite(r0.z) && radiance_finite(r1.x) &&
                            radiance_finite(r1.y) && radiance_finite(r1.z);
        const bool zero   = r1.x == 0.0f && r1.y == 0.0f && r1.z == 0.0f;
        rgb        acc    = mkc(0, 0, 0);
        if (listed && finite && !zero) {
            rng_seed_twisted(rng, __float_as_uint(r0.w));
            Ctx c{ sc, rng, q, st, 0u, 0u };
            if (args.deep) {
                c.deep    = args.deep + gwave * 64 + lane;
                c.dstride = args.deep_stride;
            }
            Ray ray;
            ray.o = mk(r0.x, r0.y, r0.z);
            ray.d = mk(r1.x, r1.y, r1.z);
            for (uint32_t s = 0; s < args.spp; ++s) {
                rng_prepare(rng);
                acc = cadd(acc, integrate<INTEG>(c, ray)); // image(p) += integrate(...)
            }
            acc = cdivs(acc, (float)args.spp); // image(p) /= num_pixel_samples
            rays_total += c.rays;
            shadow_total += c.shadow;
            samples_total += args.spp;
            draws_total += rng.draws;
        }
        if (listed) {
            float* o = args.out + (size_t)i * 3;
            o[0]     = acc.r;
            o[1]     = acc.g;
            o[2]     = acc.b;
        }
    }
    // render_tiles_body's counter reduction
    unsigned long long v[4] = { rays_total, shadow_total, samples_total, draws_total };
    for (int k = 0; k < 4; ++k) {
        unsigned long long s = v[k];
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
        if (lane == 0 && s) atomicAdd(args.counters + k, s);
    }
}

template <int INTEG, int MINW>
__global__ void __launch_bounds__(64 * WAVES_PER_BLOCK, MINW) sp_radiance_kernel(Scene sc, RenderArgs args, RadianceArgs ra)
{
    radiance_rays_body<INTEG>(sc, args, ra);
}
} // inline namespace SPD_LAYOUT_NS

// the same split as the views family (sp_mega.hpp); no Mandelbrot: it has no ray
using RadianceFn = void (*)(Scene, RenderArgs, RadianceArgs);
RadianceFn radiance_direct(int variant);
RadianceFn radiance_rrnee(int waves);
RadianceFn radiance_path(int integ);
RadianceFn select_radiance(int integ, int variant); // nullptr: Mandelbrot

} // namespace spd
