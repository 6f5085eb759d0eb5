// sp_build.hpp -- the device BVH builder (sp_build.hip): a linear BVH over primitive bounds,
// the same tree as sph::build_bvh_lbvh bit for bit.
#pragma once

#include "../host/sp_host.hpp"

#include <string>
#include <vector>

namespace spb {

struct BuildStats {
    double ms_bounds_up = 0, ms_codes = 0, ms_sort = 0, ms_hierarchy = 0, ms_fit = 0, ms_copy_back = 0;
    int    passes     = 0; // fit launches over the internal nodes
    size_t peak_bytes = 0; // device scratch alive at once, the sort's and the scan's temporaries included
};

// Builds on the current device.  SP_OK, or SP_ERR_HIP with `err` set (nothing stays allocated and
// HIP's error state is cleared; there is no host fall-back).  `timed` waits for the device after
// each stage so the stats hold stage times.
int build_lbvh_device(const std::vector<sph::PrimBounds>& bounds, int max_leaf, sph::Bvh& out, BuildStats& st,
                      std::string& err, bool timed);

} // namespace spb
