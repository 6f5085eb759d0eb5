// sp_radiance_path.hip -- radiance queries, BruteForce / BruteForceIterative(RR) / Whitted:
// sp_radiance_kernel with the default sampler options, as their one-shot kernels
// (sp_mega_recursive.hip, sp_mega_iterative.hip).
#include "sp_radiance.hpp"

namespace spd {
RadianceFn radiance_path(int integ)
{
    switch (integ) {
    case SP_INTEGRATOR_WHITTED: return sp_radiance_kernel<SP_INTEGRATOR_WHITTED, 2>;
    case SP_INTEGRATOR_BRUTE_FORCE_ITERATIVE: return sp_radiance_kernel<SP_INTEGRATOR_BRUTE_FORCE_ITERATIVE, 2>;
    case SP_INTEGRATOR_BRUTE_FORCE_ITERATIVE_RR: return sp_radiance_kernel<SP_INTEGRATOR_BRUTE_FORCE_ITERATIVE_RR, 2>;
    default: return sp_radiance_kernel<SP_INTEGRATOR_BRUTE_FORCE, 2>;
    }
}
} // namespace spd
