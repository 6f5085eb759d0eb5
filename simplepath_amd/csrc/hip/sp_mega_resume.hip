// sp_mega_resume.hip -- progressive renders (sp_progress_render): the sp_resume_kernel family's
// kernel selection, and its DirectLighting and Mandelbrot instantiations with the sampler options of
// their one-shot kernels (sp_mega_direct.hip).  The other integrators' instantiations carry their
// own options in sp_mega_resume_rrnee.hip and sp_mega_resume_path.hip.
#define SP_RNG_PF 0
#ifndef SP_RHO_TOUCH
#define SP_RHO_TOUCH 1
#endif
#ifndef SP_RNG_PAIR
#define SP_RNG_PAIR 1
#endif
#include "sp_mega.hpp"

namespace spd {
ResumeFn resume_direct(int variant)
{
    switch (variant) {
    case 1: return sp_resume_kernel<SP_INTEGRATOR_DIRECT_LIGHTING, 1>;
    case 2: return sp_resume_kernel<SP_INTEGRATOR_DIRECT_LIGHTING, 2>;
    case 3: return sp_resume_kernel<SP_INTEGRATOR_DIRECT_LIGHTING, 3>;
    default: return sp_resume_kernel<SP_INTEGRATOR_DIRECT_LIGHTING, 4>;
    }
}
ResumeFn resume_mandelbrot() { return sp_resume_kernel<SP_INTEGRATOR_MANDELBROT, 2>; }

// variant as select_kernel's (sp_mega.hip)
ResumeFn select_resume(int integ, int variant)
{
    switch (integ) {
    case SP_INTEGRATOR_BRUTE_FORCE:
    case SP_INTEGRATOR_WHITTED:
    case SP_INTEGRATOR_BRUTE_FORCE_ITERATIVE:
    case SP_INTEGRATOR_BRUTE_FORCE_ITERATIVE_RR: return resume_path(integ);
    case SP_INTEGRATOR_ITERATIVE_RRNEE: return resume_rrnee(variant);
    case SP_INTEGRATOR_MANDELBROT: return resume_mandelbrot();
    default: return resume_direct(variant);
    }
}
} // namespace spd
