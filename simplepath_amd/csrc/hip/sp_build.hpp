// sp_build.hpp -- the device BVH builder (sp_build.hip): a linear BVH over primitive bounds,
// the same tree as sph::build_bvh_lbvh bit for bit.
#pragma once

#include "../host/sp_host.hpp"

#include <hip/hip_runtime.h>

#include <string>
#include <vector>

namespace spb {

struct BuildStats {
    double ms_bounds_up = 0, ms_codes = 0, ms_sort = 0, ms_hierarchy = 0, ms_fit = 0, ms_copy_back = 0;
    int    passes     = 0; // fit launches over the internal nodes
    size_t peak_bytes = 0; // device scratch alive at once, the sort's and the scan's temporaries included
};

// A tree that stays on the device (the device finish works on it there).  It owns both blocks:
// what the caller has not taken over (sp_scene::adopt nulls the pointer it takes) is freed with it.
struct DeviceTree {
    void *   nodes = nullptr, *order = nullptr; // sph::BvhNode[n_nodes]; uint32_t[n_slots], slot -> primitive
    uint32_t n_nodes = 0, n_slots = 0;

    DeviceTree() = default;
    DeviceTree(const DeviceTree&) = delete;
    DeviceTree& operator=(const DeviceTree&) = delete;
    ~DeviceTree() { reset(); }
    void free_order() // build scratch once the finish has read it
    {
        if (order) (void)hipFree(order);
        order = nullptr;
    }
    void reset()
    {
        free_order();
        if (nodes) (void)hipFree(nodes);
        nodes   = nullptr;
        n_nodes = n_slots = 0;
    }
};

// Builds on the current device.  SP_OK, or SP_ERR_HIP with `err` set (nothing stays allocated and
// HIP's error state is cleared; there is no host fall-back).  `timed` waits for the device after
// each stage so the stats hold stage times.  With `keep` and more than one primitive the tree is
// not copied back: `keep` takes the device blocks, and `out` holds only max_depth, which is the
// fit's pass count plus one -- a node is fitted in the pass that equals its height.
int build_lbvh_device(const std::vector<sph::PrimBounds>& bounds, int max_leaf, sph::Bvh& out, BuildStats& st,
                      std::string& err, bool timed, DeviceTree* keep = nullptr);

} // namespace spb
