// sp_mega_views.hip -- many views in one launch (sp_render_views): the sp_views_kernel family's
// kernel selection, and its DirectLighting instantiations with the sampler options of their one-shot
// kernel (sp_mega_direct.hip).  The other integrators' instantiations carry their own options in
// sp_mega_views_rrnee.hip and sp_mega_views_path.hip.  Mandelbrot has no camera and no views kernel.
#define SP_RNG_PF 0
#ifndef SP_RHO_TOUCH
#define SP_RHO_TOUCH 1
#endif
#ifndef SP_RNG_PAIR
#define SP_RNG_PAIR 1
#endif
#include "sp_mega.hpp"

namespace spd {
ViewsFn views_direct(int variant)
{
    switch (variant) {
    case 1: return sp_views_kernel<SP_INTEGRATOR_DIRECT_LIGHTING, 1>;
    case 2: return sp_views_kernel<SP_INTEGRATOR_DIRECT_LIGHTING, 2>;
    case 3: return sp_views_kernel<SP_INTEGRATOR_DIRECT_LIGHTING, 3>;
    default: return sp_views_kernel<SP_INTEGRATOR_DIRECT_LIGHTING, 4>;
    }
}

// variant as select_kernel's (sp_mega.hip)
ViewsFn select_views(int integ, int variant)
{
    switch (integ) {
    case SP_INTEGRATOR_BRUTE_FORCE:
    case SP_INTEGRATOR_WHITTED:
    case SP_INTEGRATOR_BRUTE_FORCE_ITERATIVE:
    case SP_INTEGRATOR_BRUTE_FORCE_ITERATIVE_RR: return views_path(integ);
    case SP_INTEGRATOR_ITERATIVE_RRNEE: return views_rrnee(variant);
    case SP_INTEGRATOR_MANDELBROT: return nullptr;
    default: return views_direct(variant);
    }
}
} // namespace spd
