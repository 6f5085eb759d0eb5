// sp_mega_adapt.hip -- rounds and uniform passes on adaptive progress objects (sp_adaptive_round,
// sp_progress_render): the sp_adapt_kernel family's kernel selection, and its DirectLighting and
// Mandelbrot instantiations with the sampler options of their one-shot kernels (sp_mega_direct.hip),
// as sp_mega_resume.hip does for sp_resume_kernel.  The other integrators' instantiations carry
// their own options in sp_mega_adapt_rrnee.hip and sp_mega_adapt_path.hip.
#define SP_RNG_PF 0
#ifndef SP_RHO_TOUCH
#define SP_RHO_TOUCH 1
#endif
#ifndef SP_RNG_PAIR
#define SP_RNG_PAIR 1
#endif
#include "sp_mega.hpp"

namespace spd {
AdaptFn adapt_direct(int variant)
{
    switch (variant) {
    case 1: return sp_adapt_kernel<SP_INTEGRATOR_DIRECT_LIGHTING, 1>;
    case 2: return sp_adapt_kernel<SP_INTEGRATOR_DIRECT_LIGHTING, 2>;
    case 3: return sp_adapt_kernel<SP_INTEGRATOR_DIRECT_LIGHTING, 3>;
    default: return sp_adapt_kernel<SP_INTEGRATOR_DIRECT_LIGHTING, 4>;
    }
}
AdaptFn adapt_mandelbrot() { return sp_adapt_kernel<SP_INTEGRATOR_MANDELBROT, 2>; }

// variant as select_kernel's (sp_mega.hip)
AdaptFn select_adapt(int integ, int variant)
{
    switch (integ) {
    case SP_INTEGRATOR_BRUTE_FORCE:
    case SP_INTEGRATOR_WHITTED:
    case SP_INTEGRATOR_BRUTE_FORCE_ITERATIVE:
    case SP_INTEGRATOR_BRUTE_FORCE_ITERATIVE_RR: return adapt_path(integ);
    case SP_INTEGRATOR_ITERATIVE_RRNEE: return adapt_rrnee(variant);
    case SP_INTEGRATOR_MANDELBROT: return adapt_mandelbrot();
    default: return adapt_direct(variant);
    }
}
} // namespace spd
