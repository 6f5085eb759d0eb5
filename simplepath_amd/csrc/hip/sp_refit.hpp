// sp_refit.hpp -- the device refit (sp_refit.hip): new vertex positions into the
// records of a resident scene, then every box of the binary tree and every record of the 8-wide
// tree bottom-up, in place.  The topology stays; the bytes are those of the host restatement
// (sph::lbvh_fit_boxes, sph::refit_wide) on the same topology and positions.
#pragma once

#include "../host/sp_host.hpp"

#include <hip/hip_runtime.h>

#include <string>

namespace spr {

struct RefitStats {
    double ms_copy = 0, ms_pack = 0, ms_binary = 0, ms_wide = 0, ms_total = 0;
    int    binary_passes = 0, wide_passes = 0; // fit launches after the leaves' / the childless records'
    size_t peak_bytes    = 0;                  // device scratch alive at once, all freed on return
};

struct RefitIn {
    sph::BvhNode*   d_nodes     = nullptr; // device: the binary tree, boxes rewritten
    uint32_t        n_nodes     = 0;
    int             geom_depth  = 0;       // its levels (root = 1): the height of the root
    float4*         d_slot_tri  = nullptr; // device: 3 per slot, rewritten
    const uint32_t* d_slot_code = nullptr;
    uint32_t        n_slots     = 0;
    uint32_t*       d_wnodes    = nullptr; // device: 20 words per record, rewritten; null: no wide tree
    uint32_t        records     = 0;
    int             wide_depth  = 0;
    float4*         d_wslot_tri = nullptr; // device: 3 per wide slot, rewritten
    uint32_t        wide_slots  = 0;
    const uint32_t* d_indices   = nullptr; // device: three vertex indices per triangle
    size_t          n_indices   = 0;
    const spm::f3*  h_verts     = nullptr; // host: the new positions (uploaded as scratch)
    size_t          n_verts     = 0;
    const spm::f3*  h_normals   = nullptr; // host: new normals, or null
    float*          d_normals   = nullptr; // device: 3 per vertex, overwritten when h_normals is given
    const sph::PrimBounds* h_shape_bounds = nullptr; // host: bounds by shape index (spheres; planes: any)
    uint32_t        n_shapes    = 0;
};

// Runs on the current device's null stream and waits for it.  SP_OK, or SP_ERR_HIP with `err` set
// (HIP's error state is cleared; the arrays may be half rewritten: the caller gives the residency
// up).  `timed` waits for the device after each stage so the stats hold stage times.
int refit_device(const RefitIn& in, RefitStats& st, std::string& err, bool timed);

} // namespace spr
