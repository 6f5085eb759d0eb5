// sp_finish.hpp -- the device finish (sp_finish.hip): from a binary geometry BVH
// resident in device memory to every array a render reads -- wnodes, wslot_tri, slot_tri,
// slot_code, parents -- the same bytes as the host path (sph::build_wide, pack_records,
// parent_links) makes from the same tree.
#pragma once

#include "../host/sp_host.hpp"

#include <hip/hip_runtime.h>

#include <string>

namespace spf {

struct FinishStats {
    double ms_inputs_up = 0, ms_collapse = 0, ms_sums = 0, ms_bases = 0, ms_emit = 0, ms_pack = 0, ms_parents = 0;
    int    levels     = 0; // launch sets of the collapse = depth of the wide tree
    size_t peak_bytes = 0; // device scratch alive at once (the outputs are not scratch)
};

struct FinishIn {
    const sph::BvhNode* d_nodes   = nullptr; // device: the binary tree
    uint32_t            n_nodes   = 0;
    const uint32_t*     d_order   = nullptr; // device: slot -> bounded primitive; or
    const int32_t*      h_order   = nullptr; // host: the same (uploaded as scratch when d_order is null)
    uint32_t            n_slots   = 0;
    const uint32_t*     h_codes   = nullptr; // host: code of each bounded primitive (kind << 30 | index)
    uint32_t            n_prims   = 0;
    const spm::f3*      h_verts   = nullptr; // host: vertex positions (uploaded as scratch)
    size_t              n_verts   = 0;
    const uint32_t*     d_indices = nullptr; // device: three vertex indices per triangle
    size_t              n_indices = 0;
    bool                want_wide = false, want_parents = false;
};

// Device buffers for the caller to take over on SP_OK; nullptr where there is nothing.  It owns
// them: what the caller has not taken (sp_scene::adopt nulls the pointer it takes) is freed with it.
struct FinishOut {
    void *   wnodes = nullptr, *wslot_tri = nullptr, *slot_tri = nullptr, *slot_code = nullptr, *parents = nullptr;
    size_t   wnodes_bytes = 0, wslot_tri_bytes = 0, slot_tri_bytes = 0, slot_code_bytes = 0, parents_bytes = 0;
    uint32_t records = 0, wide_slots = 0;
    int      depth = 0;

    FinishOut() = default;
    FinishOut(const FinishOut&) = delete;
    FinishOut& operator=(const FinishOut&) = delete;
    ~FinishOut() { reset(); }
    void reset()
    {
        for (void** p : { &wnodes, &wslot_tri, &slot_tri, &slot_code, &parents }) {
            if (*p) (void)hipFree(*p);
            *p = nullptr;
        }
        wnodes_bytes = wslot_tri_bytes = slot_tri_bytes = slot_code_bytes = parents_bytes = 0;
        records = wide_slots = 0;
        depth   = 0;
    }
};

// Runs on the current device.  SP_OK, or SP_ERR_HIP with `err` set: nothing stays allocated and
// HIP's error state is cleared.  `timed` waits for the device after each stage.
int finish_device(const FinishIn& in, FinishOut& out, FinishStats& st, std::string& err, bool timed);

} // namespace spf
