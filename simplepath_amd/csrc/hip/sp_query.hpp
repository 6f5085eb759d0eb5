// sp_query.hpp -- arguments and host entry points of the ray-query kernels (sp_query.hip):
// sp_scene_trace_rays' closest-hit and any-hit walks over a caller's ray buffer.  Declared apart from
// sp_launch.hpp so that no translation unit of the render kernels sees them.
#pragma once
#include "sp_device.hpp"

#include <hip/hip_runtime.h>

namespace spd {

struct QueryArgs {
    const sp_ray*       rays;      // num_rays records of 32 bytes, 16-byte aligned
    int64_t             num_rays;
    sp_ray_hit*         hits;      // closest hit: one 32-byte record per ray
    float4*             normals;   // closest hit, optional: {n.x, n.y, n.z, 0} per ray
    uint32_t*           occluded;  // any hit: one word per ray
    unsigned long long* hit_count; // nullptr: not counted (no statistics asked for)
};

constexpr int QUERY_BLOCK = 256; // one lane per ray, four waves per block

// Dynamic LDS of a query block: its four waves' traversal stacks (none on a stackless scene) and,
// for closest hits with normals, the RSQRTSS table in front of them.
size_t     query_lds_bytes(const Scene& sc, bool any_hit, bool normals);
hipError_t launch_query_closest(const Scene& sc, const QueryArgs& a, size_t lds_bytes, hipStream_t stream);
hipError_t launch_query_any(const Scene& sc, const QueryArgs& a, size_t lds_bytes, hipStream_t stream);

} // namespace spd
