// sp_radiance_rrnee.hip -- radiance queries, IterativeRRNEE: sp_radiance_kernel with the sampler
// options of its one-shot kernel (sp_mega_rrnee.hip; each is measured and explained there).
#ifndef SP_SERVE_RHO
#define SP_SERVE_RHO 1
#endif
#define SP_RNG_PF 0
#define SP_RHO_TOUCH 1
#define SP_RNG_MARGIN 144
#ifndef SP_SERVE_SAMPLE
#define SP_SERVE_SAMPLE 1
#endif
#ifndef SP_SERVED_ALIGNED
#define SP_SERVED_ALIGNED 1
#endif
#ifndef SP_SERVED_TOUCH
#define SP_SERVED_TOUCH 0
#endif
#include "sp_radiance.hpp"

namespace spd {
RadianceFn radiance_rrnee(int w)
{
    if (w == 2) return sp_radiance_kernel<SP_INTEGRATOR_ITERATIVE_RRNEE, 2>;
    if (w == 4) return sp_radiance_kernel<SP_INTEGRATOR_ITERATIVE_RRNEE, 4>;
    return sp_radiance_kernel<SP_INTEGRATOR_ITERATIVE_RRNEE, 3>;
}
} // namespace spd
