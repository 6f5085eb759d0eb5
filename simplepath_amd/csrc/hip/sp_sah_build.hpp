// sp_sah_build.hpp -- the device SAH builder (sp_sah_build.hip): binned SAH over primitive bounds,
// the same tree as sph::build_bvh_sah byte for byte.
#pragma once

#include "sp_build.hpp"

namespace spb {

constexpr uint32_t SAH_SMALL_DEFAULT = 128; // a node of at most this many primitives is built by one thread
constexpr uint32_t SAH_SMALL_MIN = 4, SAH_SMALL_MAX = 65536;
constexpr int      SAH_BLOCK = 256;          // slots per workgroup of the level kernels

struct SahStats {
    double   ms_bounds_up = 0, ms_levels = 0, ms_subtrees = 0, ms_number = 0, ms_emit = 0, ms_copy_back = 0;
    int      levels     = 0; // level-wise passes over the open nodes
    uint32_t top_nodes  = 0; // nodes split by the level kernels
    uint32_t subtrees   = 0; // ranges handed to one thread each
    size_t   peak_bytes = 0; // device scratch alive at once, the scan's temporary included
};

// Builds on the current device.  SP_OK; SP_ERR_UNSUPPORTED when a bound is not finite (the tree of
// such input depends on the order of the folds; nothing is built); or SP_ERR_HIP with `err` set.
// In every failure nothing stays allocated and HIP's error state is cleared; there is no host
// fall-back.  `timed` waits for the device after each stage.  With `keep` and more than one
// primitive the tree is not copied back: `keep` takes the device blocks and `out` holds only
// max_depth.  `small`: the hand-over size (0: the default), clamped to [SAH_SMALL_MIN, SAH_SMALL_MAX];
// the tree does not depend on it.
int build_sah_device(const std::vector<sph::PrimBounds>& bounds, int max_leaf, sph::Bvh& out, SahStats& st, std::string& err,
                     bool timed, DeviceTree* keep = nullptr, uint32_t small = 0);

} // namespace spb
