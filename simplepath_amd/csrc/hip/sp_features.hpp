// sp_features.hpp -- arguments and host entry points of the feature kernels (sp_features.hip):
// sp_scene_camera_rays (the render's camera rays, exported) and sp_scene_features (first-hit
// features reduced per pixel over those rays).  Declared apart from sp_launch.hpp so that no
// translation unit of the render kernels sees them.
#pragma once
#include "sp_device.hpp"

#include <hip/hip_runtime.h>

namespace spd {

// One wave per tile slot, one lane per pixel (the megakernel's Morton lane order).
struct CameraRayArgs {
    const int32_t* tile_ids;     // nullptr => identity
    int64_t        num_tiles;
    int32_t        tiles_x;
    uint32_t       first_sample; // the R2 index of record s = 0
    uint32_t       num_samples;
    sp_ray*        rays;         // [num_tiles][num_samples][64] records of 32 bytes, 16-byte aligned
};

struct FeatureArgs {
    const int32_t*      tile_ids;     // nullptr => identity
    int64_t             num_tiles;
    int32_t             tiles_x;
    uint32_t            spp;          // every slot's sample count, unless
    const uint32_t*     tile_samples; // [num_tiles] per-slot counts (nullptr: spp)
    int4*               ids;          // [slot][64] {kind, index, material of sample 0's hit, |H|}; any of the five may be nullptr
    float*              coverage;     // [slot][64]
    float*              depth;        // [slot][64]
    float*              normal;       // [slot][64][3]
    float*              albedo;       // [slot][64][3]
    unsigned long long* counters;     // {camera rays, hits}; nullptr: not counted (no statistics asked for)
};

constexpr int FEATURE_BLOCK = 256; // four waves = four tile slots per block

// Dynamic LDS of a feature block: the RSQRTSS table (the camera ray's normalize reads it) and its
// four waves' traversal stacks (none on a stackless scene) -- a shading block's layout.
size_t     feature_lds_bytes(const Scene& sc);
hipError_t launch_camera_rays(const Scene& sc, const CameraRayArgs& a, hipStream_t stream);
hipError_t launch_features(const Scene& sc, const FeatureArgs& a, size_t lds_bytes, hipStream_t stream);

} // namespace spd
