// sp_envbuild.hpp -- the image light's tables built on the device (sp_envbuild.hip):
// what the ImageBasedEnvironmentLight constructor derives from its pixels -- the clamped radiance
// image, the Distribution2D over the 2x luminance x sin(theta) image, the guide tables -- written
// into device blocks the caller owns.  The bytes are those of sph::build_env_map (sp_envmap.cpp),
// the host restatement, from the same pixels.
#pragma once

#include "../host/sp_host.hpp"

#include <hip/hip_runtime.h>

#include <string>

namespace spe {

struct EnvBuildStats {
    double ms_upload = 0, ms_clamp = 0, ms_func = 0, ms_rows = 0, ms_marginal = 0, ms_guides = 0, ms_total = 0;
    size_t peak_bytes = 0; // device scratch alive at once, all freed on return
};

// sizes of the tables of a w x h map, in elements
struct EnvSizes {
    size_t texels, func, cdf, rows, marg_cdf, cond_guide, marg_guide;
    int    nu, nv, cond_bits, marg_bits;
};
EnvSizes env_sizes(int w, int h);

struct EnvBuildIn {
    int          w = 0, h = 0;
    float        max_radiance = 0.0f;
    const float* h_pixels = nullptr; // host, w * h * 3 (uploaded as scratch), or
    const float* d_pixels = nullptr; // device, the same layout
    // device blocks of env_sizes(w, h) elements, all written
    float4* radiance  = nullptr;
    float * cond_func = nullptr, *cond_cdf = nullptr, *cond_int = nullptr, *marg_func = nullptr, *marg_cdf = nullptr;
    // written only when every row and the marginal are ordered; null: the guides are not wanted
    uint32_t *cond_guide = nullptr, *marg_guide = nullptr;
};

struct EnvBuildOut {
    float marg_int = 0.0f;
    bool  guided   = false; // every cdf[0..n-1] is non-decreasing (no NaN): what the host calls guided
};

// Runs on the current device's null stream and waits for it.  SP_OK, or SP_ERR_HIP with `err` set
// (HIP's error state is cleared; the blocks may be half written: the caller gives the residency up).
// `timed` waits for the device after each stage so the stats hold stage times.
int build_env_device(const EnvBuildIn& in, EnvBuildOut& out, EnvBuildStats& st, std::string& err, bool timed);

} // namespace spe
