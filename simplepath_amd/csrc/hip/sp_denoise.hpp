// sp_denoise.hpp -- arguments and host entry points of the denoiser's kernels (sp_denoise.hip):
// the edge-avoiding a-trous filter of include/simplepath_hip.h ("denoising") on tile-packed frames.
// Scene-free: no translation unit of the render kernels sees this, and this one sees none of them.
#pragma once
#include "../common/sp_denoise.h"

#include <hip/hip_runtime.h>

namespace spd {

// One wave per tile slot, one lane per pixel in Morton order (the image's own layout).
struct DenoiseArgs {
    const int32_t* tile_ids;     // the object's copy of the list; nullptr => identity
    const int32_t* slot_of_tile; // [tiles_x * tiles_y]: the lowest slot that lists the tile, -1: absent
    int64_t        num_tiles;
    int32_t        tiles_x, tiles_y, width, height;
    const float*   color;        // [slot][64][3]
    const float*   albedo;       // [slot][64][3] or nullptr
    const float*   normal;       // [slot][64][3] or nullptr
    const float*   depth;        // [slot][64] or nullptr
    const float*   coverage;     // [slot][64] or nullptr
    float*         out;          // [slot][64][3]; may be `color`
    float4*        plane[2];     // [slot][64] {x0, x1, x2, z}: level i reads plane[i & 1], writes the other
    float4*        guide;        // [slot][64] {n0, n1, n2, k}
    float          sigma_depth, depth_floor, albedo_floor; // the floors resolved (never 0 for "default")
    int32_t        demodulate;
    unsigned long long* counters; // {pixels inside the image, counted taps}; nullptr: not counted
};

constexpr int DENOISE_BLOCK = 256; // four waves = four tile slots per block

// slot_of_tile, preset to -1 by the caller: atomicMin of the slots that list each tile
hipError_t launch_denoise_map(const int32_t* tile_ids, int64_t num_tiles, int32_t total_tiles, int32_t* slot_of_tile,
                              hipStream_t stream);
hipError_t launch_denoise_prepare(const DenoiseArgs& a, hipStream_t stream);
// level `i` of `levels`; the last one finishes (remodulates) into a.out
hipError_t launch_denoise_level(const DenoiseArgs& a, const spdn::Level& L, int i, int levels, hipStream_t stream);

} // namespace spd
