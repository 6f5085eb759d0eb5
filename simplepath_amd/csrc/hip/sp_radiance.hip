// sp_radiance.hip -- radiance queries (sp_scene_radiance_rays): the sp_radiance_kernel family's
// kernel selection and launch, and its DirectLighting instantiations with the sampler options of
// their one-shot kernel (sp_mega_direct.hip).  The other integrators' instantiations carry their own
// options in sp_radiance_rrnee.hip and sp_radiance_path.hip.  Mandelbrot has no ray and no kernel.
#define SP_RNG_PF 0
#ifndef SP_RHO_TOUCH
#define SP_RHO_TOUCH 1
#endif
#ifndef SP_RNG_PAIR
#define SP_RNG_PAIR 1
#endif
#include "sp_radiance.hpp"

namespace spd {
RadianceFn radiance_direct(int variant)
{
    switch (variant) {
    case 1: return sp_radiance_kernel<SP_INTEGRATOR_DIRECT_LIGHTING, 1>;
    case 2: return sp_radiance_kernel<SP_INTEGRATOR_DIRECT_LIGHTING, 2>;
    case 3: return sp_radiance_kernel<SP_INTEGRATOR_DIRECT_LIGHTING, 3>;
    default: return sp_radiance_kernel<SP_INTEGRATOR_DIRECT_LIGHTING, 4>;
    }
}

// variant as select_kernel's (sp_mega.hip)
RadianceFn select_radiance(int integ, int variant)
{
    switch (integ) {
    case SP_INTEGRATOR_BRUTE_FORCE:
    case SP_INTEGRATOR_WHITTED:
    case SP_INTEGRATOR_BRUTE_FORCE_ITERATIVE:
    case SP_INTEGRATOR_BRUTE_FORCE_ITERATIVE_RR: return radiance_path(integ);
    case SP_INTEGRATOR_ITERATIVE_RRNEE: return radiance_rrnee(variant);
    case SP_INTEGRATOR_MANDELBROT: return nullptr;
    default: return radiance_direct(variant);
    }
}

const void* radiance_kernel(int integ, int variant) { return reinterpret_cast<const void*>(select_radiance(integ, variant)); }

hipError_t launch_radiance(const Scene& sc, const RenderArgs& args, const RadianceArgs& ra, int integ, int variant, int blocks,
                           size_t lds_bytes, hipStream_t stream)
{
    const RadianceFn k = select_radiance(integ, variant);
    if (!ra.rays || ra.num_rays <= 0 || !args.out || args.num_tiles != (ra.num_rays + 63) / 64) return hipErrorInvalidValue;
    if (!k) return hipErrorInvalidDeviceFunction; // (an integrator without a radiance kernel: no fall-back)
    hipLaunchKernelGGL(k, dim3(blocks), dim3(64 * WAVES_PER_BLOCK), lds_bytes, stream, sc, args, ra);
    return hipGetLastError();
}
} // namespace spd
