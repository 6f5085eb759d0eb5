// sp_capi.hip -- extern "C" boundary (include/simplepath_hip.h) and HBM residency of scenes.
#include "sp_device.hpp"
#include "sp_rsqrt_pack.hpp"
#include "sp_wave.hpp"
#include "sp_chunk.hpp"
#include "sp_launch.hpp"
#include "sp_plan.hpp"
#include "sp_build.hpp"
#include "sp_sah_build.hpp"
#include "sp_finish.hpp"
#include "sp_refit.hpp"
#include "sp_query.hpp"
#include "sp_features.hpp"
#include "sp_denoise.hpp"
#include "sp_envbuild.hpp"
#include "../common/sp_refit.h"
#include "../common/sp_sah.h"
#include "../host/sp_host.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

namespace {
thread_local std::string g_last_error;

int fail(int code, const std::string& msg)
{
    g_last_error = msg;
    return code;
}

#define SP_HIP(call)                                                                                      \
    do {                                                                                                  \
        hipError_t e__ = (call);                                                                          \
        if (e__ != hipSuccess) return fail(SP_ERR_HIP, std::string(#call ": ") + hipGetErrorString(e__)); \
    } while (0)

constexpr int MAX_RECURSION = 32; // sp_path.hpp integrate_bruteforce / integrate_whitted in-register levels

uint32_t code_of(int kind, int index) { return ((uint32_t)kind << spd::CODE_SHIFT) | (uint32_t)index; }

// BBox3 of a primitive (shapes/Triangle.h:228, shapes/Shape.h:290 for transformed shapes)
sph::PrimBounds tri_bounds(const sph::Scene& s, int t)
{
    // BBox::extend per vertex, min(p, m_min): spr::tri_box (sp_refit.h), shared with the device refit
    const spm::f3*  v   = s.vertices.data();
    const spr::Box  box = spr::tri_box(&v[s.indices[3 * t]].x, &v[s.indices[3 * t + 1]].x, &v[s.indices[3 * t + 2]].x);
    sph::PrimBounds b;
    for (int i = 0; i < 3; ++i) { b.lo[i] = box.lo[i]; b.hi[i] = box.hi[i]; }
    return b;
}

spm::aff from_desc(const sp_affine& d)
{
    spm::aff a;
    a.vx = spm::mk(d.vx[0], d.vx[1], d.vx[2]);
    a.vy = spm::mk(d.vy[0], d.vy[1], d.vy[2]);
    a.vz = spm::mk(d.vz[0], d.vz[1], d.vz[2]);
    a.p  = spm::mk(d.p[0], d.p[1], d.p[2]);
    return a;
}
spm::lin from_desc(const sp_linear& d)
{
    spm::lin a;
    a.vx = spm::mk(d.vx[0], d.vx[1], d.vx[2]);
    a.vy = spm::mk(d.vy[0], d.vy[1], d.vy[2]);
    a.vz = spm::mk(d.vz[0], d.vz[1], d.vz[2]);
    return a;
}

sph::PrimBounds sphere_bounds(const spm::aff& o2w)
{
    sph::PrimBounds b;
    for (int i = 0; i < 3; ++i) { b.lo[i] = INFINITY; b.hi[i] = -INFINITY; }
    // AffineSpace::operator()(BBox3) (math/AffineSpace.h:104): corners p0..p7
    const float lo = -1.0f, hi = 1.0f;
    const float cs[8][3] = { { lo, lo, lo }, { lo, lo, hi }, { lo, hi, lo }, { lo, hi, hi },
                             { hi, lo, lo }, { hi, lo, hi }, { hi, hi, lo }, { hi, hi, hi } };
    for (auto& c : cs) {
        const spm::f3 p    = spm::xfm_point(o2w, spm::mk(c[0], c[1], c[2]));
        const float   v[3] = { p.x, p.y, p.z };
        for (int i = 0; i < 3; ++i) {
            b.lo[i] = spm::sse_min(v[i], b.lo[i]);
            b.hi[i] = spm::sse_max(v[i], b.hi[i]);
        }
    }
    return b;
}

// Accelerator options of an upload (sp_upload_params, ABI 4): explicit fields win; fields left
// automatic take the SP_* environment overrides (test hooks), else the measured defaults.
struct UploadOpts {
    int  bvh_mode   = 0;
    bool stackless  = false; // forced parent-link walk
    int  stack_max  = 96;    // deepest BVH (levels) walked with the LDS stack
    bool wide       = true;  // 8-wide any-hit BVH on SAH scenes
    bool env_guide  = true;  // image-light guide tables
    bool wide_closest = true;  // closest-hit queries on the 8-wide BVH as well
    int  sah_leaf   = 4;
    int  builder    = SP_BUILDER_HOST; // SP_BUILDER_HOST, _DEVICE or _DEVICE_SAH (sp_build_params, resolved)
    int  finish     = SP_FINISH_HOST;  // SP_FINISH_HOST or SP_FINISH_DEVICE (sp_build_params_ex, resolved)
    bool operator==(const UploadOpts& o) const
    {
        return bvh_mode == o.bvh_mode && stackless == o.stackless && stack_max == o.stack_max && wide == o.wide &&
               env_guide == o.env_guide && sah_leaf == o.sah_leaf && wide_closest == o.wide_closest && builder == o.builder &&
               finish == o.finish;
    }
};

// The SP_* test hooks of the upload path, read once per call (the struct's initialisers are the
// compiled defaults).  All but the last three stand in for an sp_upload_params / sp_build_params field
// left automatic; `sah_small`, `timing` and `rsqrt_pack` have no field, and are not part of UploadOpts:
// a change of SP_RSQRT_PACK alone does not make an upload with the resident options build again, and
// SP_SAH_SMALL does not reach the tree at all.
struct UploadHooks {
    int  stackless = 0, stack_max = 96, wide = 1, env_guide = 1, wide_closest = 1, sah_leaf = 4;
    int  device_build = 0, device_finish = -1; // -1: the finish follows the builder
    int  device_env   = 0;                     // SP_DEVICE_ENV=1: the image lights' tables from the device builder (sp_envbuild.hip)
    int  sah_small    = 0;                     // SP_SAH_SMALL: the device SAH builder's hand-over size (0: its default)
    bool timing     = false;                   // SP_UPLOAD_TIMING (set at all): the sp_upload_timing line
    bool rsqrt_pack = true;                    // SP_RSQRT_PACK=0: 32-bit RSQRTSS entries (comparison)

    static UploadHooks from_env()
    {
        UploadHooks h;
        int         pack = 1;
        const std::pair<const char*, int*> ints[] = {
            { "SP_STACKLESS", &h.stackless }, { "SP_STACK_MAX", &h.stack_max }, { "SP_WIDE", &h.wide },
            { "SP_ENV_GUIDE", &h.env_guide }, { "SP_WIDE_CLOSEST", &h.wide_closest }, { "SP_SAH_LEAF", &h.sah_leaf },
            { "SP_DEVICE_BUILD", &h.device_build }, { "SP_DEVICE_FINISH", &h.device_finish }, { "SP_SAH_SMALL", &h.sah_small },
            { "SP_DEVICE_ENV", &h.device_env },
            { "SP_RSQRT_PACK", &pack } };
        for (const auto& e : ints)
            if (const char* v = std::getenv(e.first)) *e.second = std::atoi(v);
        h.timing     = std::getenv("SP_UPLOAD_TIMING") != nullptr;
        h.rsqrt_pack = pack != 0;
        return h;
    }
};

int resolve_upload(const sp_upload_params* p, const UploadHooks& hooks, UploadOpts& o)
{
    const sp_upload_params z{};
    if (!p) p = &z;
    if (p->reserved != 0) return fail(SP_ERR_ARG, "sp_upload_params.reserved must be 0");
    if (p->binary_closest != 0 && p->binary_closest != 1) return fail(SP_ERR_ARG, "binary_closest must be 0 or 1");
    if (p->bvh_mode != 0 && p->bvh_mode != 1) return fail(SP_ERR_ARG, "bvh_mode must be 0 (SAH) or 1 (reference)");
    if (p->walk != SP_WALK_AUTO && p->walk != SP_WALK_STACKLESS) return fail(SP_ERR_ARG, "walk must be SP_WALK_AUTO or SP_WALK_STACKLESS");
    if (p->stack_max_levels < 0) return fail(SP_ERR_ARG, "stack_max_levels < 0");
    if (p->sah_leaf < 0 || p->sah_leaf > 4) return fail(SP_ERR_ARG, "sah_leaf must be 0 (automatic) or 1..4");
    o.bvh_mode  = p->bvh_mode;
    o.stackless = p->walk == SP_WALK_STACKLESS || (p->walk == SP_WALK_AUTO && hooks.stackless != 0);
    o.stack_max = p->stack_max_levels ? p->stack_max_levels : std::max(1, hooks.stack_max);
    o.wide      = !p->no_wide_bvh && hooks.wide != 0;
    o.env_guide = !p->env_replay && hooks.env_guide != 0;
    o.wide_closest = !p->binary_closest && hooks.wide_closest != 0;
    // SAH leaf size limit (1..4: 8 collapsed leaves of a wide node must fit its 5-bit leaf
    // offsets; the sweep in DESIGN.md §4 found 4 best)
    o.sah_leaf  = p->sah_leaf ? p->sah_leaf : std::max(1, std::min(4, hooks.sah_leaf));
    return SP_OK;
}

// The builder of an upload (sp_build_params): NULL or AUTO is the host builders, unless the test
// hook SP_DEVICE_BUILD=1 (linear BVH) or =2 (device SAH) asks for a device builder on a SAH-mode upload.  The finish
// (sp_build_params_ex, told apart by struct_size): AUTO follows the builder unless the test hook
// SP_DEVICE_FINISH=0|1 decides.  sp_upload_params is validated first.
int resolve_opts(const sp_upload_params* p, const sp_build_params* b, const UploadHooks& hooks, UploadOpts& o)
{
    if (int rc = resolve_upload(p, hooks, o)) return rc;
    int builder = SP_BUILDER_AUTO, finish = SP_FINISH_AUTO;
    if (b) {
        if (b->struct_size != sizeof(sp_build_params) && b->struct_size != sizeof(sp_build_params_ex))
            return fail(SP_ERR_ARG, "sp_build_params.struct_size is not a known size");
        if (b->reserved[0] != 0 || b->reserved[1] != 0) return fail(SP_ERR_ARG, "sp_build_params.reserved must be 0");
        if (b->struct_size == sizeof(sp_build_params_ex)) {
            const sp_build_params_ex* x = reinterpret_cast<const sp_build_params_ex*>(b);
            if (x->reserved2[0] != 0 || x->reserved2[1] != 0 || x->reserved2[2] != 0)
                return fail(SP_ERR_ARG, "sp_build_params_ex.reserved2 must be 0");
            if (x->finish != SP_FINISH_AUTO && x->finish != SP_FINISH_HOST && x->finish != SP_FINISH_DEVICE)
                return fail(SP_ERR_ARG, "finish must be SP_FINISH_AUTO, SP_FINISH_HOST or SP_FINISH_DEVICE");
            finish = x->finish;
        }
        if (b->builder != SP_BUILDER_AUTO && b->builder != SP_BUILDER_HOST && b->builder != SP_BUILDER_DEVICE &&
            b->builder != SP_BUILDER_DEVICE_SAH)
            return fail(SP_ERR_ARG, "builder must be SP_BUILDER_AUTO, SP_BUILDER_HOST, SP_BUILDER_DEVICE or SP_BUILDER_DEVICE_SAH");
        builder = b->builder;
    }
    if ((builder == SP_BUILDER_DEVICE || builder == SP_BUILDER_DEVICE_SAH) && o.bvh_mode == 1)
        return fail(SP_ERR_ARG, "the device builders cannot make the reference order (bvh_mode 1)");
    if (builder == SP_BUILDER_AUTO)
        builder = o.bvh_mode != 0 ? SP_BUILDER_HOST
                  : hooks.device_build == 1 ? SP_BUILDER_DEVICE
                  : hooks.device_build == 2 ? SP_BUILDER_DEVICE_SAH
                                            : SP_BUILDER_HOST;
    o.builder = builder;
    if (finish == SP_FINISH_DEVICE && o.bvh_mode == 1)
        return fail(SP_ERR_ARG, "the device finish cannot serve the reference order (bvh_mode 1)");
    if (finish == SP_FINISH_AUTO) {
        const int  hook = hooks.device_finish;
        const bool dev  = hook == 0 ? false : (hook == 1 ? true : builder == SP_BUILDER_DEVICE || builder == SP_BUILDER_DEVICE_SAH);
        finish         = (dev && o.bvh_mode == 0) ? SP_FINISH_DEVICE : SP_FINISH_HOST;
    }
    o.finish = finish;
    return SP_OK;
}

// Scene ctor partition (base/Scene.h:29: bounded primitives first, planes after, libstdc++
// std::partition order) and the bounds of the bounded part
std::vector<sph::PrimBounds> bounded_prims(const sph::Scene& h, std::vector<int32_t>& prims, size_t& part)
{
    prims.resize(h.prim_kind.size());
    for (size_t i = 0; i < prims.size(); ++i) prims[i] = (int32_t)i;
    part = sph::stl_partition(prims, 0, prims.size(), [&](int32_t p) { return h.prim_kind[p] != SP_PRIM_PLANE; });
    std::vector<sph::PrimBounds> bounds;
    bounds.reserve(part);
    for (size_t i = 0; i < part; ++i) {
        const int32_t p = prims[i];
        if (h.prim_kind[p] == SP_PRIM_TRIANGLE) bounds.push_back(tri_bounds(h, h.prim_index[p]));
        else bounds.push_back(sphere_bounds(from_desc(h.shapes[h.prim_index[p]].object_to_world)));
    }
    return bounds;
}

// One upload's stage times (tools/upload_timing.py): printed as a JSON line when SP_UPLOAD_TIMING is set
struct UploadTiming {
    double          ms_bounds = 0, ms_bvh = 0, ms_wide = 0, ms_pack = 0, ms_copies = 0;
    spb::BuildStats dev{};
    spb::SahStats   sah{};
    spf::FinishStats fin{};
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void lap(double& ms)
    {
        const auto t1 = std::chrono::steady_clock::now();
        ms += std::chrono::duration<double, std::milli>(t1 - t0).count();
        t0 = t1;
    }
};

// How a render walks the scene's accelerators (spd::Scene carries these five)
struct WalkPlan {
    bool stackless = false, wide_closest = false; // parent links, no stack; closest hits on the 8-wide BVH too
    int  stack_depth = 0, stack_words = 0, any_stack_words = 0; // LDS words per lane
};

// The walk of a scene from its options and the depths of its trees.  wide_depth 0: no 8-wide BVH (one
// that exists has a record and a level, from either finish: its depth says as much as its record
// count); `stackless` depends on the binary depths alone, so it is known before the wide tree, which
// is built only for a scene that keeps its stack.
// Traversal-stack budget: a BVH deeper than stack_max levels (default 96) is walked without a
// stack (parent links, sp_path.hpp bvh_next) instead of failing.  96 entries x 4 B x 64 lanes x 4
// waves = 96 KB of LDS, which leaves room for the 16 KB RSQRTSS table and a second block per CU.
// Words of LDS traversal stack per lane: the binary walks push at most one deferred child per
// level; the wide walks one child group per level, and the closest-hit form keeps each group's
// entry distance in the upper half.  SAH scenes walk the 8-wide BVH for every query (any-hit since
// round 1, closest hit since round 3: DESIGN.md §9g); then no query walks the binary geometry BVH,
// so its depth no longer sizes the stack -- only the wide and the light BVH's do (lucy 30 -> 22
// words: a fourth 4-wave block fits a CU's LDS).
WalkPlan walk_plan(const UploadOpts& o, int geom_depth, int light_depth, int wide_depth)
{
    WalkPlan w;
    w.stackless = o.stackless || std::max(geom_depth, light_depth) + 1 > o.stack_max;
    if (w.stackless) return w; // deeper than the LDS budget: no stack words at all
    w.wide_closest = o.wide_closest && wide_depth != 0;
    w.stack_depth  = w.wide_closest ? std::max(2 * (wide_depth + 1), light_depth + 1)
                                    : std::max(geom_depth, std::max(wide_depth, light_depth)) + 1;
    w.stack_words     = w.stack_depth;
    w.any_stack_words = std::max(wide_depth == 0 ? geom_depth : wide_depth, light_depth) + 1;
    return w;
}

// Per-slot primitive records in the binary tree's order: slot_code, and slot_tri = 3 x float4 with
// the triangle's vertices (zero for other primitives) and the code in p0.w, so a triangle test is
// three 16-byte fetches
void pack_records(const sph::Scene& h, const std::vector<int32_t>& prims, const std::vector<int32_t>& prim_order,
                  std::vector<float4>& slot_tri, std::vector<uint32_t>& slot_code)
{
    slot_tri.assign(prim_order.size() * 3, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    slot_code.resize(prim_order.size());
    for (size_t sl = 0; sl < prim_order.size(); ++sl) {
        const int32_t p    = prims[prim_order[sl]];
        const int     kind = h.prim_kind[p];
        const int     idx  = h.prim_index[p];
        slot_code[sl]      = code_of(kind, idx);
        if (kind == SP_PRIM_TRIANGLE) {
            for (int k = 0; k < 3; ++k) {
                const spm::f3 v  = h.vertices[h.indices[3 * idx + k]];
                slot_tri[3 * sl + k] = make_float4(v.x, v.y, v.z, 0.0f);
            }
        }
        uint32_t code = slot_code[sl];
        std::memcpy(&slot_tri[3 * sl].w, &code, 4);
    }
}

// parent[i] of every node of a binary BVH (the root is its own parent)
std::vector<uint32_t> parent_links(const std::vector<sph::BvhNode>& nodes)
{
    std::vector<uint32_t> par(nodes.size(), 0u);
    for (size_t i = 0; i < nodes.size(); ++i) {
        if (nodes[i].b & sph::BVH_LEAF) continue;
        par[nodes[i].a & sph::BVH_CHILD_MASK] = (uint32_t)i;
        par[nodes[i].b]                       = (uint32_t)i;
    }
    return par;
}

// Everything the host knows about a scene's accelerators under given options: build_trees fills the
// first half, finish_host the arrays a render reads (for the callers that want them made here).
struct HostAccel {
    std::vector<int32_t>         prims, lids; // Scene ctor order: `part` bounded primitives, `lpart` sphere lights first
    size_t                       part = 0, lpart = 0;
    std::vector<sph::PrimBounds> bounds;       // of the bounded primitives
    sph::Bvh                     bvh, lbvh;    // geometry (only max_depth when the tree stays on the device), lights
    size_t                       n_nodes = 0, n_slots = 0; // the geometry tree's, wherever it is
    bool                         want_wide = false;
    WalkPlan                     walk; // after build_trees as for no wide tree (stackless is final); then with its depth
    sph::WideBvh                 wide;
    std::vector<float4>          slot_tri, wslot_tri;
    std::vector<uint32_t>        slot_code, parents, light_parents;
};

enum class BuildOn { HOST, DEVICE }; // where a device builder runs: its host restatement, or the current device

// Scene ctor's light accelerator (base/Scene.h:29): sphere lights first (libstdc++
// std::partition order), the reference BVH over them; the rest are unbounded.  An upload's, and
// sp_scene_set_lights' on a resident scene.
void build_light_tree(const std::vector<sp_light_desc>& lights, HostAccel& a)
{
    a.lids.resize(lights.size());
    for (size_t i = 0; i < a.lids.size(); ++i) a.lids[i] = (int32_t)i;
    a.lpart = sph::stl_partition(a.lids, 0, a.lids.size(), [&](int32_t i) { return lights[i].kind == SP_LIGHT_SPHERE; });
    std::vector<sph::PrimBounds> lb;
    for (size_t i = 0; i < a.lpart; ++i) lb.push_back(sphere_bounds(from_desc(lights[a.lids[i]].object_to_world)));
    a.lbvh = sph::build_bvh_reference(lb);
}

// Bounds; the BVH over the bounded part -- the reference's median split (bvh_mode 1,
// shapes/BVHAccelerator.h:173), binned SAH, or the linear BVH of the device builder (one tree,
// from the device or its host restatement); the light BVH; and from their depths whether the scene
// is walked without a stack (then with the light tree's parent links, which either finish needs)
// or gets the 8-wide BVH (SAH scenes; no_wide_bvh keeps the binary walk).  With `keep` (device
// builder and device finish) the geometry tree stays on the device, in `keep`.
void build_trees(const sph::Scene& h, HostAccel& a, const UploadOpts& o, BuildOn where, UploadTiming* tm = nullptr,
                 spb::DeviceTree* keep = nullptr, int sah_small = 0)
{
    a.bounds = bounded_prims(h, a.prims, a.part);
    if (tm) tm->lap(tm->ms_bounds);
    if (o.bvh_mode == 1) a.bvh = sph::build_bvh_reference(a.bounds);
    else if (o.builder == SP_BUILDER_DEVICE_SAH) {
        // the host's SAH tree from the device (sp_sah_build.hip) or its level-wise restatement;
        // both refuse bounds that are not finite, whose tree depends on the order of the folds
        if (where == BuildOn::HOST) {
            for (const sph::PrimBounds& b : a.bounds)
                if (!sah::finite_bounds(b.lo, b.hi)) throw sph::SpError(SP_ERR_UNSUPPORTED, "device SAH build: a primitive's bounds are not finite");
            a.bvh = sph::build_bvh_sah_levels(a.bounds, o.sah_leaf);
        } else {
            spb::SahStats st;
            std::string   err;
            const int     rc = spb::build_sah_device(a.bounds, o.sah_leaf, a.bvh, tm ? tm->sah : st, err, tm != nullptr, keep,
                                                     (uint32_t)std::max(0, sah_small));
            if (rc != SP_OK) throw sph::SpError(rc, err);
        }
    } else if (o.builder != SP_BUILDER_DEVICE) a.bvh = sph::build_bvh_sah(a.bounds, o.sah_leaf);
    else if (where == BuildOn::HOST) a.bvh = sph::build_bvh_lbvh(a.bounds, o.sah_leaf);
    else {
        spb::BuildStats st;
        std::string     err;
        const int       rc = spb::build_lbvh_device(a.bounds, o.sah_leaf, a.bvh, tm ? tm->dev : st, err, tm != nullptr, keep);
        if (rc != SP_OK) throw sph::SpError(rc, err);
    }
    const bool kept = keep && keep->nodes;
    a.n_nodes       = kept ? keep->n_nodes : a.bvh.nodes.size();
    a.n_slots       = kept ? keep->n_slots : a.bvh.prim_order.size();
    if (tm) tm->lap(tm->ms_bvh);
    build_light_tree(h.lights, a);
    a.walk      = walk_plan(o, a.bvh.max_depth, a.lbvh.max_depth, 0);
    a.want_wide = o.bvh_mode != 1 && o.wide && a.n_nodes != 0 && !a.walk.stackless;
    if (a.walk.stackless) a.light_parents = parent_links(a.lbvh.nodes);
    if (tm) tm->lap(tm->ms_copies); // (lights: counted with the copies)
}

// The host finish: records, the 8-wide tree with its own copy of the records in its slot order,
// and the geometry tree's parent links for a stackless walk.  The level-wise collapse stands in
// for the device finish (the same bytes: tests/golden/wide_hashes.json).
void finish_host(const sph::Scene& h, HostAccel& a, const UploadOpts& o, UploadTiming* tm = nullptr)
{
    pack_records(h, a.prims, a.bvh.prim_order, a.slot_tri, a.slot_code);
    if (a.walk.stackless) a.parents = parent_links(a.bvh.nodes);
    if (tm) tm->lap(tm->ms_pack);
    if (a.want_wide) {
        a.wide = o.finish == SP_FINISH_DEVICE ? sph::build_wide_levels(a.bvh) : sph::build_wide(a.bvh);
        if (tm) tm->lap(tm->ms_wide);
        a.wslot_tri.resize(a.wide.slot_of.size() * 3);
        for (size_t i = 0; i < a.wide.slot_of.size(); ++i)
            for (int k = 0; k < 3; ++k) a.wslot_tri[3 * i + k] = a.slot_tri[3 * (size_t)a.wide.slot_of[i] + k];
        if (tm) tm->lap(tm->ms_pack);
    }
    a.walk = walk_plan(o, a.bvh.max_depth, a.lbvh.max_depth, a.wide.depth);
}

static_assert(splan::MT_N == spm::MT_N && splan::MT_GEN_WORDS == spd::MT_GEN_WORDS && splan::WF_MAX_LIGHTS == spd::WF_MAX_LIGHTS,
              "sp_plan.hpp's copies of the layout constants");

// Grow-only scratch memory, device or pinned host.  reserve() does nothing when the capacity
// suffices; otherwise it frees the old block BEFORE it allocates the new one -- the chunk and tail
// budgets (free device memory + this buffer's capacity) count on that, and a 20 GB store must never
// exist twice.  A failed allocation leaves the buffer empty (no pointer, no capacity: the next call
// allocates again instead of trusting a stale size) and clears HIP's sticky error.
template <bool PINNED>
struct Scratch {
    void*  ptr = nullptr;
    size_t cap = 0; // bytes

    Scratch() = default;
    Scratch(const Scratch&) = delete;
    Scratch(Scratch&& o) noexcept { *this = std::move(o); }
    Scratch& operator=(Scratch&& o) noexcept // (o's destructor frees what this held)
    {
        std::swap(ptr, o.ptr);
        std::swap(cap, o.cap);
        return *this;
    }
    ~Scratch() { reset(); }
    void reset()
    {
        if (ptr) (void)(PINNED ? hipHostFree(ptr) : hipFree(ptr));
        ptr = nullptr;
        cap = 0;
    }
    hipError_t reserve(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        reset();
        const hipError_t e = PINNED ? hipHostMalloc(&ptr, bytes, hipHostMallocDefault) : hipMalloc(&ptr, bytes);
        if (e != hipSuccess) {
            ptr = nullptr;
            (void)hipGetLastError();
            return e;
        }
        cap = bytes;
        return hipSuccess;
    }
    template <typename T>
    T* as() const { return static_cast<T*>(ptr); }
};
using DeviceScratch = Scratch<false>;
using PinnedScratch = Scratch<true>;

// The *_host forms: render n_tiles tiles into a temporary device image, then copy it to h_out
template <typename Render>
int render_to_host(int64_t n_tiles, float* h_out, Render&& render)
{
    const size_t  bytes = n_tiles > 0 ? (size_t)n_tiles * 64 * 3 * sizeof(float) : 0; // (< 0: the render refuses)
    DeviceScratch d;
    SP_HIP(d.reserve(std::max<size_t>(bytes, 4)));
    int rc = render(d.as<float>());
    if (rc == SP_OK && bytes) {
        hipError_t e = hipMemcpy(h_out, d.ptr, bytes, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(SP_ERR_HIP, hipGetErrorString(e));
    }
    return rc;
}

// N events or streams, created where they are first needed (a null entry: not yet) and destroyed with their owner
template <typename H, hipError_t (*DESTROY)(H), int N = 1>
struct Handles {
    H h[N] = {};

    Handles() = default;
    Handles(const Handles&) = delete;
    Handles(Handles&& o) noexcept { *this = std::move(o); }
    Handles& operator=(Handles&& o) noexcept
    {
        std::swap(h, o.h);
        return *this;
    }
    ~Handles()
    {
        for (H x : h)
            if (x) (void)DESTROY(x);
    }
    operator H() const { return h[0]; }
    H& operator[](int i) { return h[i]; }
};
template <int N = 1>
using Events = Handles<hipEvent_t, hipEventDestroy, N>;
template <int N = 1>
using Streams = Handles<hipStream_t, hipStreamDestroy, N>;

// a growing list of timing events (SP_RENDER_STAGE_TIMING)
struct EventList {
    std::vector<hipEvent_t> v;

    EventList() = default;
    EventList(const EventList&) = delete;
    EventList& operator=(EventList&& o) noexcept
    {
        v.swap(o.v);
        return *this;
    }
    ~EventList()
    {
        for (hipEvent_t e : v) (void)hipEventDestroy(e);
    }
};

// Everything a scene's render calls keep on the device between calls.  Each member frees itself:
// sp_scene::release() assigns an empty one, and a new member needs no second edit.
struct RenderScratch {
    static constexpr int STAGE_RING = 4; // sp_scene: the staging ring of host tile lists

    DeviceScratch mt_state;     // the megakernel's generator store, per persistent wave
    DeviceScratch tile_counter; // int32: the persistent queue's head
    DeviceScratch counters;     // 8 x u64: rays, shadow rays, samples, draws, primary hits
    DeviceScratch d_tiles;      // a host tile list's device copy
    DeviceScratch wave_buf;     // wavefront pipeline state (sp_wave.hpp WaveArgs)
    DeviceScratch ck_buf;       // sample-chunk pipeline: hits, radiance, snapshots
    DeviceScratch ck_ctr;       // 2 x int32
    DeviceScratch deep_buf;     // recursive integrators beyond MAX_RECURSION levels
    // megakernel tile order: probe times, queue order -- a pair that grows together (order_tiles)
    DeviceScratch d_tile_time, d_order;
    DeviceScratch probe_counters;
    DeviceScratch tail_buf;     // megakernel tail chunks: TailArgs, flags, hits, radiance, store
    EventList     stage_ev;     // SP_RENDER_STAGE_TIMING
    Streams<spd::WF_MAX_PARTS - 1> aux_stream; // parts 1.. of the wavefront pipeline
    Events<>      ev_fork;
    Events<spd::WF_MAX_PARTS - 1>  ev_join;
    Events<spd::WF_MAX_PARTS>      ev_shade;
    Events<>      ev0, ev1;
    Events<>      ev_render;    // megakernel, stage timing: before the render launch
    Events<>      ev_done;      // recorded at the end of every render call
    bool          done_rec = false;
    PinnedScratch h_tiles[STAGE_RING];    // pinned staging of host tile lists
    Events<STAGE_RING> ev_tiles;          // after each buffer's staged copy
    bool          tiles_rec[STAGE_RING] = {};
    int           stage_next = 0;
    // sp_render_views: a call's host cameras, staged as the tile lists are (a ring of its own)
    DeviceScratch d_cams;
    PinnedScratch h_cams[STAGE_RING];
    Events<STAGE_RING> ev_cams;
    bool          cams_rec[STAGE_RING] = {};
    int           cams_next = 0;
    int           n_cu = 0;    // the device's compute units (0: not asked yet)
};

// The device blocks of the parts of a resident scene that an edit replaces (sp_scene_set_lights,
// sp_scene_set_env_image): each block is as large as its array, so an edited scene holds the
// bytes a fresh upload of the edited scene would.
struct LightBlocks {
    DeviceScratch lights, unbounded, nodes, slot, parents;
    size_t bytes() const { return lights.cap + unbounded.cap + nodes.cap + slot.cap + parents.cap; }
};
struct EnvBlocks {
    DeviceScratch radiance, cond_func, cond_cdf, cond_int, marg_func, marg_cdf, cond_guide, marg_guide;
    int  builder = SP_ENV_BUILDER_HOST; // who made the tables
    bool guided  = false;               // rows and marginal ordered (the guide blocks exist only if the upload wants them too)
    size_t bytes() const
    {
        return radiance.cap + cond_func.cap + cond_cdf.cap + cond_int.cap + marg_func.cap + marg_cdf.cap + cond_guide.cap + marg_guide.cap;
    }
};

// Sizes of the resident accelerators: what the check and info calls need to read them back
struct ResidentSizes {
    int    geom_depth = 0, light_depth = 0, wide_depth = 0;
    size_t geom_nodes = 0, geom_slots = 0;
    size_t wide_records = 0, wide_slots = 0; // 8-wide BVH (0: none)
};
} // namespace

struct sp_scene {
    std::unique_ptr<sph::Scene> host;
    sp_scene_desc               desc{};
    std::vector<sp_env_image>   env_descs; // desc.env_images
    std::vector<sp_material_desc> mat_descs; // desc.materials
    // device residency
    int                  device   = -1; // >= 0 only after an upload that built everything
    UploadOpts           opts{};    // effective accelerator options of the resident upload
    std::vector<DeviceScratch> bufs; // every device array of the resident scene that no edit replaces
    LightBlocks          light_blocks; // lights and their accelerator
    std::vector<EnvBlocks>   env_blocks; // per env image, its tables
    std::vector<spd::EnvMap> env_recs;   // the host's copy of dev.envs
    DeviceScratch        env_recs_buf;
    spd::Scene           dev{};
    ResidentSizes        sizes;
    // One scene, many host threads (the reference's render() shares one Scene across N threads,
    // main.cpp:122-130): the render scratch is per scene, so calls are serialised -- on the
    // host by `mu`, and on the device by making each call's stream wait for the previous call's
    // last operation (ev_done), whichever stream that call used.  A host tile list is staged
    // through a ring of STAGE_RING pinned buffers (h_tiles), each rewritten only once its previous
    // copy has run, so the caller's array may be reused as soon as sp_render_tiles returns.  Each
    // staged copy is queued behind the previous call's render (ev_done), so with one buffer a third
    // back-to-back call waited on the host for the first render; with the ring the host waits only
    // when STAGE_RING calls are queued ahead of the copy it needs.
    std::mutex           mu;
    RenderScratch        scratch;
    // counts every change that invalidates a progress object made on this scene (sp_progress):
    // a new upload (the device scene is rebuilt), sp_scene_set_resolution, sp_scene_update_mesh and
    // sp_scene_set_camera (an object's kept tile order is the old camera's)
    uint64_t             generation = 0;
    // the resident trees were refitted (sp_scene_update_mesh): their topology is an earlier pose's, so
    // an upload with the resident options builds again instead of finding the scene resident
    bool                 refitted = false;

    void release()
    {
        refitted = false;
        if (device >= 0) (void)hipSetDevice(device);
        bufs.clear();
        light_blocks = LightBlocks{};
        env_blocks.clear();
        env_recs.clear();
        env_recs_buf.reset();
        scratch = RenderScratch{};
        sizes   = ResidentSizes{};
        dev     = spd::Scene{};
        device  = -1;
    }
    ~sp_scene() { release(); }

    // takes over a device block made elsewhere (sp_build.hip, sp_finish.hip): `p` is null afterwards
    template <typename T>
    void adopt(void*& p, size_t bytes, const T** out)
    {
        *out = static_cast<const T*>(p);
        if (!p) return;
        bufs.emplace_back(); // (first: a failed push leaves `p` with its owner)
        bufs.back().ptr = p;
        bufs.back().cap = bytes;
        p               = nullptr;
    }

    template <typename T>
    int upload(const std::vector<T>& v, const T** out)
    {
        *out = nullptr;
        if (v.empty()) return SP_OK;
        bufs.emplace_back();
        SP_HIP(bufs.back().reserve(v.size() * sizeof(T)));
        SP_HIP(hipMemcpy(bufs.back().ptr, v.data(), bufs.back().cap, hipMemcpyHostToDevice));
        *out = bufs.back().as<T>();
        return SP_OK;
    }

    // `v` into a block of exactly its size: the block is kept when the size is, else made again
    template <typename T>
    int put(DeviceScratch& b, const std::vector<T>& v, const T** out)
    {
        *out = nullptr;
        if (v.empty()) {
            b.reset();
            return SP_OK;
        }
        const size_t bytes = v.size() * sizeof(T);
        if (b.cap != bytes) {
            b.reset();
            SP_HIP(b.reserve(bytes));
        }
        SP_HIP(hipMemcpy(b.ptr, v.data(), bytes, hipMemcpyHostToDevice));
        *out = b.as<T>();
        return SP_OK;
    }
    size_t device_bytes() const
    {
        size_t b = light_blocks.bytes() + env_recs_buf.cap;
        for (const auto& d : bufs) b += d.cap;
        for (const auto& e : env_blocks) b += e.bytes();
        return b;
    }
};

// Progressive render (include/simplepath_hip.h): the carried per-pixel state of one tile list, in
// device memory this object owns.  Layout: sp_device.hpp ResumeArgs.
struct sp_progress {
    sp_scene*            scene      = nullptr;
    uint64_t             generation = 0; // the scene's when this was created
    int                  device     = -1;
    int32_t              integ      = 0;
    int                  waves_req  = 0;
    float                order_factor = 0.0f;
    bool                 listed     = false;
    int64_t              n_tiles    = 0;
    int32_t              width = 0, height = 0;
    std::vector<int32_t> h_ids;          // the list (host copy; empty: slot = tile)
    int32_t*             d_ids   = nullptr;
    spd::ResumeArgs      st{};           // gen / pos / draws / sum; n0 = samples done
    float*               d_tile_time = nullptr; // tile order, probed by the first call and kept
    int32_t*             d_order     = nullptr;
    bool                 order_tried = false, ordered = false;
    int64_t              bytes = 0;
    // adaptive objects (sp_progress_create_adaptive): per-tile counts and per-pixel noise statistics;
    // st.n0 is then only an upper bound of the tile counts (the device holds the counts)
    bool                 adaptive = false;
    spd::AdaptArgs       ad{};
    std::vector<uint8_t> h_inside;       // per slot, its pixels inside the image
    // every device array above comes from alloc() and lives here (freeing one waits for the kernels
    // that still use it)
    std::vector<DeviceScratch> mem;

    // `bytes` of device memory this object owns, zeroed when asked
    template <typename T>
    hipError_t alloc(T** out, size_t n_bytes, bool zero = true)
    {
        mem.emplace_back();
        if (hipError_t e = mem.back().reserve(n_bytes)) return e;
        *out = mem.back().as<T>();
        bytes += (int64_t)n_bytes;
        return zero ? hipMemset(*out, 0, n_bytes) : hipSuccess;
    }
    ~sp_progress()
    {
        if (device >= 0) (void)hipSetDevice(device);
    }
};

namespace {
void fill_desc(sp_scene* s)
{
    const sph::Scene& h = *s->host;
    sp_scene_desc&    d = s->desc;
    d                   = sp_scene_desc{};
    d.info.image_width  = h.image_width;
    d.info.image_height = h.image_height;
    d.info.russian_roulette_depth = h.rr_depth;
    d.info.max_depth              = h.max_depth;
    d.info.integrator_type        = h.integrator;
    d.info.num_triangles          = static_cast<int32_t>(h.tri_material.size());
    d.info.num_vertices           = static_cast<int32_t>(h.vertices.size());
    d.info.num_shapes             = static_cast<int32_t>(h.shapes.size());
    d.info.num_lights             = static_cast<int32_t>(h.lights.size());
    d.info.num_materials          = static_cast<int32_t>(h.materials.size());
    std::strncpy(d.info.output_file_name, h.output_file_name.c_str(), sizeof(d.info.output_file_name) - 1);
    auto put = [](float* o, spm::f3 v) { o[0] = v.x; o[1] = v.y; o[2] = v.z; };
    put(d.camera.transform.vx, h.camera.vx);
    put(d.camera.transform.vy, h.camera.vy);
    put(d.camera.transform.vz, h.camera.vz);
    put(d.camera.transform.p, h.camera.p);
    d.camera.film_width  = h.image_width;
    d.camera.film_height = h.image_height;
    static_assert(sizeof(spm::f3) == 12, "f3 packing");
    d.vertices     = h.vertices.empty() ? nullptr : &h.vertices[0].x;
    d.normals      = h.normals.empty() ? nullptr : &h.normals[0].x;
    d.indices      = h.indices.empty() ? nullptr : h.indices.data();
    d.tri_material = h.tri_material.empty() ? nullptr : h.tri_material.data();
    d.shapes       = h.shapes.empty() ? nullptr : h.shapes.data();
    d.prim_kind    = h.prim_kind.empty() ? nullptr : h.prim_kind.data();
    d.prim_index   = h.prim_index.empty() ? nullptr : h.prim_index.data();
    d.num_prims    = static_cast<int64_t>(h.prim_kind.size());
    d.lights       = h.lights.empty() ? nullptr : h.lights.data();
    s->env_descs.clear();
    for (const auto& e : h.env_images) {
        sp_env_image x{};
        x.width        = e.width;
        x.height       = e.height;
        x.pixels       = e.pixels.data();
        x.max_radiance = e.max_radiance;
        put(x.light_to_world.vx, e.light_to_world.vx);
        put(x.light_to_world.vy, e.light_to_world.vy);
        put(x.light_to_world.vz, e.light_to_world.vz);
        put(x.world_to_light.vx, e.world_to_light.vx);
        put(x.world_to_light.vy, e.world_to_light.vy);
        put(x.world_to_light.vz, e.world_to_light.vz);
        s->env_descs.push_back(x);
    }
    s->mat_descs.clear();
    for (const auto& m : h.materials) s->mat_descs.push_back(m.d);
    d.materials      = s->mat_descs.empty() ? nullptr : s->mat_descs.data();
    d.env_images     = s->env_descs.empty() ? nullptr : s->env_descs.data();
    d.num_env_images = static_cast<int32_t>(s->env_descs.size());
}

int wrap_load(std::unique_ptr<sph::Scene> (*fn)(const std::string&, const std::string&), const std::string& a,
              const std::string& b, sp_scene** out)
{
    try {
        auto* s = new sp_scene;
        s->host = fn(a, b);
        fill_desc(s);
        *out = s;
        return SP_OK;
    } catch (const sph::SpError& e) {
        return fail(e.code, e.what());
    } catch (const std::exception& e) {
        return fail(SP_ERR_PARSE, std::string("Unexpected file parsing error: ") + e.what());
    }
}
} // namespace

extern "C" {

const char* sp_version(void) { return "simplepath-amd 0.1 (gfx950)"; }
// content hash of the sources and flags of this build (simplepath_amd/Makefile, ABI 5)
extern const char* const sp_build_id_str;
const char* sp_build_id(void) { return sp_build_id_str; }
const char* sp_last_error(void) { return g_last_error.c_str(); }

int sp_string_to_integrator(const char* name, int32_t* out)
{
    if (!name || !out) return fail(SP_ERR_ARG, "null argument");
    std::string s(name);
    while (!s.empty() && std::isspace(static_cast<unsigned char>(s.back()))) s.pop_back();
    size_t b = 0;
    while (b < s.size() && std::isspace(static_cast<unsigned char>(s[b]))) ++b;
    s = s.substr(b);
    // Integrators/Integrator.cpp:25 string_to_integrator_type
    if (s == "mandelbrot") *out = SP_INTEGRATOR_MANDELBROT;
    else if (s == "brute_force") *out = SP_INTEGRATOR_BRUTE_FORCE;
    else if (s == "brute_force_iterative") *out = SP_INTEGRATOR_BRUTE_FORCE_ITERATIVE;
    else if (s == "brute_force_iterative_rr") *out = SP_INTEGRATOR_BRUTE_FORCE_ITERATIVE_RR;
    else if (s == "iterative_rrnee") *out = SP_INTEGRATOR_ITERATIVE_RRNEE;
    else if (s == "direct_lighting") *out = SP_INTEGRATOR_DIRECT_LIGHTING;
    else if (s == "whitted") *out = SP_INTEGRATOR_WHITTED;
    else return fail(SP_ERR_ARG, "Unknown integrator type");
    return SP_OK;
}

int sp_scene_load(const char* path, sp_scene** out)
{
    if (!path || !out) return fail(SP_ERR_ARG, "null argument");
    return wrap_load([](const std::string& p, const std::string&) { return sph::parse_scene_file(p); }, path, "", out);
}

int sp_scene_load_string(const char* text, const char* base_dir, sp_scene** out)
{
    if (!text || !out) return fail(SP_ERR_ARG, "null argument");
    return wrap_load(&sph::parse_scene, text, base_dir ? base_dir : ".", out);
}

void sp_scene_free(sp_scene* scene) { delete scene; }

int sp_scene_get_info(const sp_scene* scene, sp_scene_info* out)
{
    if (!scene || !out) return fail(SP_ERR_ARG, "null argument");
    *out = scene->desc.info;
    return SP_OK;
}

int sp_scene_get_desc(const sp_scene* scene, sp_scene_desc* out)
{
    if (!scene || !out) return fail(SP_ERR_ARG, "null argument");
    *out = scene->desc; // arrays owned by the scene: valid until sp_scene_free
    return SP_OK;
}

// A host that already built its scene (the reference's main.cpp:368-395 holds an sp::Scene)
// hands it over flattened; nothing is re-parsed.  Every array is copied and checked.
static int scene_from_desc_impl(const sp_scene_desc* d, sp_scene** out)
{
    if (!d || !out) return fail(SP_ERR_ARG, "null argument");
    const sp_scene_info& in = d->info;
    if (in.image_width <= 0 || in.image_height <= 0 || in.image_width > 65535 || in.image_height > 65535)
        return fail(SP_ERR_ARG, "sp_scene_desc: bad image size");
    if (in.num_triangles < 0 || in.num_vertices < 0 || in.num_shapes < 0 || in.num_lights < 0 || in.num_materials < 0 ||
        d->num_prims < 0 || d->num_env_images < 0)
        return fail(SP_ERR_ARG, "sp_scene_desc: negative count");
    auto need = [](const void* p, int64_t n) { return n == 0 || p != nullptr; };
    if (!need(d->vertices, in.num_vertices) || !need(d->normals, in.num_vertices) || !need(d->indices, in.num_triangles) ||
        !need(d->tri_material, in.num_triangles) || !need(d->shapes, in.num_shapes) || !need(d->prim_kind, d->num_prims) ||
        !need(d->prim_index, d->num_prims) || !need(d->lights, in.num_lights) || !need(d->materials, in.num_materials) ||
        !need(d->env_images, d->num_env_images))
        return fail(SP_ERR_ARG, "sp_scene_desc: null array with a nonzero count");
    if (in.integrator_type < SP_INTEGRATOR_NOT_SPECIFIED || in.integrator_type > SP_INTEGRATOR_WHITTED)
        return fail(SP_ERR_ARG, "sp_scene_desc: unknown integrator type");
    auto h             = std::make_unique<sph::Scene>();
    h->image_width     = in.image_width;
    h->image_height    = in.image_height;
    h->rr_depth        = in.russian_roulette_depth;
    h->max_depth       = in.max_depth;
    h->integrator      = in.integrator_type;
    h->output_file_name = std::string(in.output_file_name, strnlen(in.output_file_name, sizeof(in.output_file_name)));
    h->has_camera      = true;
    h->camera_fixed    = true;
    h->camera          = from_desc(d->camera.transform);
    h->vertices.resize((size_t)in.num_vertices);
    h->normals.resize((size_t)in.num_vertices);
    for (int32_t i = 0; i < in.num_vertices; ++i) {
        h->vertices[i] = spm::mk(d->vertices[3 * i], d->vertices[3 * i + 1], d->vertices[3 * i + 2]);
        h->normals[i]  = spm::mk(d->normals[3 * i], d->normals[3 * i + 1], d->normals[3 * i + 2]);
    }
    h->indices.assign(d->indices, d->indices + (size_t)in.num_triangles * 3);
    for (uint32_t v : h->indices)
        if (v >= (uint32_t)in.num_vertices) return fail(SP_ERR_ARG, "sp_scene_desc: vertex index out of range");
    h->tri_material.assign(d->tri_material, d->tri_material + in.num_triangles);
    for (int32_t m : h->tri_material)
        if (m < 0 || m >= in.num_materials) return fail(SP_ERR_ARG, "sp_scene_desc: triangle material out of range");
    h->shapes.assign(d->shapes, d->shapes + in.num_shapes);
    for (const auto& x : h->shapes) {
        if (x.kind != SP_PRIM_SPHERE && x.kind != SP_PRIM_PLANE) return fail(SP_ERR_ARG, "sp_scene_desc: bad shape kind");
        if (x.material < 0 || x.material >= in.num_materials) return fail(SP_ERR_ARG, "sp_scene_desc: shape material out of range");
    }
    h->prim_kind.assign(d->prim_kind, d->prim_kind + d->num_prims);
    h->prim_index.assign(d->prim_index, d->prim_index + d->num_prims);
    for (int64_t i = 0; i < d->num_prims; ++i) {
        const int k = h->prim_kind[i], x = h->prim_index[i];
        const int n = (k == SP_PRIM_TRIANGLE) ? in.num_triangles : in.num_shapes;
        if ((k != SP_PRIM_TRIANGLE && k != SP_PRIM_SPHERE && k != SP_PRIM_PLANE) || x < 0 || x >= n ||
            (k != SP_PRIM_TRIANGLE && h->shapes[x].kind != k))
            return fail(SP_ERR_ARG, "sp_scene_desc: bad primitive reference");
    }
    for (int32_t i = 0; i < in.num_materials; ++i) {
        const sp_material_desc& m = d->materials[i];
        if (m.kind < SP_MAT_LAMBERTIAN || m.kind > SP_MAT_CLEARCOAT ||
            (m.kind == SP_MAT_CLEARCOAT && (m.base < 0 || m.base >= in.num_materials)))
            return fail(SP_ERR_ARG, "sp_scene_desc: bad material");
        h->materials.push_back(sph::Material{ m });
        h->material_names.push_back(std::string());
    }
    for (int32_t i = 0; i < d->num_env_images; ++i) {
        const sp_env_image& e = d->env_images[i];
        if (e.width <= 0 || e.height <= 0 || !e.pixels) return fail(SP_ERR_ARG, "sp_scene_desc: bad environment image");
        sph::EnvImage x;
        x.width        = e.width;
        x.height       = e.height;
        x.pixels.assign(e.pixels, e.pixels + (size_t)e.width * e.height * 3);
        x.max_radiance = e.max_radiance;
        x.light_to_world = from_desc(e.light_to_world);
        x.world_to_light = from_desc(e.world_to_light);
        h->env_images.push_back(std::move(x));
    }
    h->lights.assign(d->lights, d->lights + in.num_lights);
    for (const auto& l : h->lights) {
        if (l.kind < SP_LIGHT_SPHERE || l.kind > SP_LIGHT_IMAGE_ENVIRONMENT) return fail(SP_ERR_ARG, "sp_scene_desc: bad light kind");
        if (l.kind == SP_LIGHT_IMAGE_ENVIRONMENT && (l.image < 0 || l.image >= d->num_env_images))
            return fail(SP_ERR_ARG, "sp_scene_desc: light image out of range");
    }
    auto* s = new sp_scene;
    s->host = std::move(h);
    fill_desc(s);
    *out = s;
    return SP_OK;
}

int sp_scene_from_desc(const sp_scene_desc* d, sp_scene** out)
{
    try {
        return scene_from_desc_impl(d, out);
    } catch (const std::exception& e) {
        return fail(SP_ERR_ARG, std::string("sp_scene_from_desc: ") + e.what());
    }
}

int sp_scene_set_resolution(sp_scene* scene, int32_t width, int32_t height)
{
    if (!scene || width <= 0 || height <= 0 || width > 65535 || height > 65535) return fail(SP_ERR_ARG, "bad resolution");
    if (scene->host->camera_fixed && (width != scene->host->image_width || height != scene->host->image_height))
        return fail(SP_ERR_STATE, "scene built from a descriptor: its camera transform fixes the image size");
    scene->host->image_width  = width;
    scene->host->image_height = height;
    if (!scene->host->camera_fixed) scene->host->rebuild_camera(); // (a given transform has no attributes to rebuild from)
    ++scene->generation;
    fill_desc(scene);
    if (scene->device >= 0) {
        scene->dev.width  = width;
        scene->dev.height = height;
        scene->dev.camera = scene->host->camera;
    }
    return SP_OK;
}

// ---- camera edits (SP_HAS_CAMERA_EDIT) ------------------------------------------------------------

static bool camera_finite(const sp_camera_desc& c)
{
    const sp_affine& t = c.transform;
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(t.vx[k]) || !std::isfinite(t.vy[k]) || !std::isfinite(t.vz[k]) || !std::isfinite(t.p[k])) return false;
    return true;
}

int sp_camera_look_at(const float eye[3], const float look_at[3], const float up[3], float fov_degrees, int32_t width,
                      int32_t height, sp_camera_desc* out)
{
    if (!eye || !look_at || !up || !out) return fail(SP_ERR_ARG, "null argument");
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(eye[k]) || !std::isfinite(look_at[k]) || !std::isfinite(up[k]))
            return fail(SP_ERR_ARG, "sp_camera_look_at: non-finite input");
    if (!std::isfinite(fov_degrees)) return fail(SP_ERR_ARG, "sp_camera_look_at: non-finite input");
    if (width < 1 || height < 1 || width > 65535 || height > 65535) return fail(SP_ERR_ARG, "sp_camera_look_at: bad film size");
    if (!(fov_degrees > 0.0f && fov_degrees < 180.0f)) return fail(SP_ERR_ARG, "sp_camera_look_at: fov_degrees outside (0, 180)");
    const spm::aff a = sph::perspective_camera_transform(spm::mk(eye[0], eye[1], eye[2]), spm::mk(look_at[0], look_at[1], look_at[2]),
                                                         spm::mk(up[0], up[1], up[2]), fov_degrees, width, height);
    auto put = [](float* o, spm::f3 v) { o[0] = v.x; o[1] = v.y; o[2] = v.z; };
    *out = sp_camera_desc{};
    put(out->transform.vx, a.vx);
    put(out->transform.vy, a.vy);
    put(out->transform.vz, a.vz);
    put(out->transform.p, a.p);
    out->film_width  = width;
    out->film_height = height;
    return SP_OK;
}

// The device side of the camera is the twelve floats of spd::Scene::camera, which every launch
// carries by value (MegaSetup::sc_run and its like): replacing them touches no device memory, and
// launches already queued keep their copy.  Nothing in RenderScratch depends on the camera; a
// progress object's kept tile order does, and the generation bump retires those objects.
int sp_scene_set_camera(sp_scene* scene, const sp_camera_desc* camera)
{
    if (!scene || !camera) return fail(SP_ERR_ARG, "null argument");
    if (camera->film_width != scene->host->image_width || camera->film_height != scene->host->image_height)
        return fail(SP_ERR_ARG, "sp_scene_set_camera: the film size is not the scene's image size");
    if (!camera_finite(*camera)) return fail(SP_ERR_ARG, "sp_scene_set_camera: non-finite transform");
    std::lock_guard<std::mutex> lock(scene->mu);
    scene->host->camera       = from_desc(camera->transform);
    scene->host->has_camera   = true;
    scene->host->camera_fixed = true;
    fill_desc(scene);
    ++scene->generation;
    if (scene->device >= 0) scene->dev.camera = scene->host->camera;
    return SP_OK;
}

int sp_tile_count(int32_t width, int32_t height, int64_t* out)
{
    if (!out || width < 0 || height < 0) return fail(SP_ERR_ARG, "bad argument");
    *out = (int64_t)((width + 7) / 8) * ((height + 7) / 8);
    return SP_OK;
}

int sp_tile_origin(int32_t width, int32_t height, int64_t tile, int32_t* x0, int32_t* y0)
{
    int64_t n;
    sp_tile_count(width, height, &n);
    if (tile < 0 || tile >= n || !x0 || !y0) return fail(SP_ERR_ARG, "tile out of range");
    const int32_t w = (width + 7) / 8;
    *x0             = (int32_t)(tile % w) * 8;
    *y0             = (int32_t)(tile / w) * 8;
    return SP_OK;
}

int sp_device_count(int32_t* out)
{
    if (!out) return fail(SP_ERR_ARG, "null argument");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *out = n;
    return SP_OK;
}

int sp_rsqrt_table_info(int32_t* mantissa_bits, int32_t* verified)
{
    const auto& c = sph::rsqrt_capture();
    if (mantissa_bits) *mantissa_bits = c.bits;
    if (verified) *verified = c.verified ? 1 : 0;
    return SP_OK;
}

int sp_rsqrt_table_get(uint32_t* entries, int64_t capacity, int32_t* bits, uint32_t* zero_result,
                       uint32_t* denorm_result)
{
    const auto& c = sph::rsqrt_active();
    if (c.entries.empty()) return fail(SP_ERR_UNSUPPORTED, "RSQRTSS table capture failed");
    if (bits) *bits = c.bits;
    if (zero_result) *zero_result = c.zero_result;
    if (denorm_result) *denorm_result = c.denorm_result;
    if (entries) {
        if (capacity < (int64_t)c.entries.size()) return fail(SP_ERR_ARG, "RSQRTSS table: capacity too small");
        std::memcpy(entries, c.entries.data(), c.entries.size() * sizeof(uint32_t));
    }
    return SP_OK;
}

int sp_rsqrt_table_set(const uint32_t* entries, int32_t bits, uint32_t zero_result, uint32_t denorm_result)
{
    try {
        sph::rsqrt_set_override(entries, bits, zero_result, denorm_result);
        return SP_OK;
    } catch (const sph::SpError& e) {
        return fail(e.code, e.what());
    }
}

float sp_host_rsqrt_emulated(float x)
{
    const auto&     c = sph::rsqrt_capture();
    spm::RsqrtTable t{ c.entries.data(), c.bits, c.zero_result, c.denorm_result };
    return spm::rsqrtss_emulated(x, t);
}

// ---- sp_scene_upload* -----------------------------------------------------------------------------

// One upload, resolved: what its steps share
struct UploadCall {
    sp_scene*       s;
    int             device;
    UploadHooks     hooks;
    UploadOpts      opts;
    UploadTiming    timing;
    UploadTiming*   tm = nullptr; // &timing under SP_UPLOAD_TIMING
    HostAccel       accel;
    spb::DeviceTree dtree; // device builder + device finish: the binary tree never comes back
    bool device_finish() const { return opts.finish == SP_FINISH_DEVICE; }
};
#define SP_TRY(call) do { if (int rc__ = (call)) return rc__; } while (0)

// Arguments, in the order their errors are promised: (the scene, by the caller,) sp_upload_params,
// sp_build_params, the device count, the device's range.  Changes no state.  `resident`: nothing to do.
static int validate_upload(UploadCall& c, const sp_upload_params* params, const sp_build_params* build, bool& resident)
{
    SP_TRY(resolve_opts(params, build, c.hooks, c.opts));
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(SP_ERR_HIP, "no HIP device");
    if (c.device < 0 || c.device >= ndev) return fail(SP_ERR_ARG, "device out of range");
    resident = c.s->device == c.device && c.s->opts == c.opts && !c.s->refitted;
    return SP_OK;
}

// (nested clearcoat is not produced by the scenes on this path)
static int convert_materials(const sph::Scene& h, std::vector<spd::Material>& mats)
{
    for (auto& m : h.materials) {
        spd::Material x{};
        x.kind           = m.d.kind;
        x.base           = m.d.base;
        x.lambert_albedo = spm::mkc(m.d.lambert_albedo[0], m.d.lambert_albedo[1], m.d.lambert_albedo[2]);
        x.microfacet_r   = spm::mkc(m.d.microfacet_r[0], m.d.microfacet_r[1], m.d.microfacet_r[2]);
        x.alpha_x        = m.d.alpha_x;
        x.alpha_y        = m.d.alpha_y;
        x.microfacet_ior = m.d.microfacet_ior;
        x.sample_visible_area = m.d.sample_visible_area;
        x.coat_ior       = m.d.coat_ior;
        x.coat_color     = spm::mkc(m.d.coat_color[0], m.d.coat_color[1], m.d.coat_color[2]);
        if (x.kind == SP_MAT_CLEARCOAT && h.materials[x.base].d.kind == SP_MAT_CLEARCOAT)
            return fail(SP_ERR_UNSUPPORTED, "clearcoat over clearcoat");
        mats.push_back(x);
    }
    return SP_OK;
}

static std::vector<spd::Shape> convert_shapes(const sph::Scene& h)
{
    std::vector<spd::Shape> shapes;
    for (auto& sh : h.shapes) {
        spd::Shape x{};
        x.o2w      = from_desc(sh.object_to_world);
        x.w2o      = from_desc(sh.world_to_object);
        x.nrm      = from_desc(sh.normal_to_world);
        x.material = sh.material;
        x.kind     = sh.kind;
        shapes.push_back(x);
    }
    return shapes;
}

static std::vector<spd::Light> convert_lights(const sph::Scene& h) // Scene::m_lights order
{
    std::vector<spd::Light> lights;
    for (auto& l : h.lights) {
        spd::Light x{};
        x.kind     = l.kind;
        x.image    = l.kind == SP_LIGHT_IMAGE_ENVIRONMENT ? l.image : -1;
        x.radiance = spm::mkc(l.radiance[0], l.radiance[1], l.radiance[2]);
        x.o2w      = from_desc(l.object_to_world);
        x.w2o      = from_desc(l.world_to_object);
        x.nrm      = from_desc(l.normal_to_world);
        lights.push_back(x);
    }
    return lights;
}

// The lights and the light accelerator (partition by boundedness: unbounded lights, nodes, slot ->
// light, parent links when stackless) of `a`, into the scene's light blocks
static int upload_lights(sp_scene* s, const HostAccel& a)
{
    const sph::Scene& h = *s->host;
    spd::Scene&       d = s->dev;
    LightBlocks&      b = s->light_blocks;
    d.n_lights = (int)h.lights.size();
    SP_TRY(s->put(b.lights, convert_lights(h), &d.lights));
    std::vector<int32_t>  unbounded_lights(a.lids.begin() + (long)a.lpart, a.lids.end());
    std::vector<uint32_t> light_slot(a.lbvh.prim_order.size());
    for (size_t sl = 0; sl < light_slot.size(); ++sl) light_slot[sl] = (uint32_t)a.lids[a.lbvh.prim_order[sl]];
    std::vector<spd::Node> lnodes(a.lbvh.nodes.size());
    std::memcpy(lnodes.data(), a.lbvh.nodes.data(), lnodes.size() * sizeof(spd::Node));
    d.n_unbounded_lights = (int)unbounded_lights.size();
    SP_TRY(s->put(b.unbounded, unbounded_lights, &d.unbounded_lights));
    d.n_light_nodes = (int)lnodes.size();
    SP_TRY(s->put(b.nodes, lnodes, &d.light_nodes));
    SP_TRY(s->put(b.slot, light_slot, &d.light_slot));
    return s->put(b.parents, a.light_parents, &d.light_parents); // (empty unless stackless)
}

// Camera, the unbounded list, the binary tree (adopted where the device built it), normals, indices
// (the device finish reads them), triangle materials, shapes, lights and the light accelerator
static int upload_scene_arrays(UploadCall& c)
{
    const sph::Scene& h = *c.s->host;
    const HostAccel&  a = c.accel;
    spd::Scene&       d = c.s->dev;
    d.camera    = h.camera;
    d.width     = h.image_width;
    d.height    = h.image_height;
    d.max_depth = h.max_depth;
    d.rr_depth  = h.rr_depth;
    float a1[1], a2[2];
    sph::rsequence_alphas(a1, a2);
    d.alpha2_0 = a2[0];
    d.alpha2_1 = a2[1];
    std::vector<int32_t> unbounded;
    for (size_t i = a.part; i < a.prims.size(); ++i) unbounded.push_back(h.prim_index[a.prims[i]]);
    d.n_unbounded = (int)unbounded.size();
    SP_TRY(c.s->upload(unbounded, &d.unbounded));
    d.n_nodes = (int)a.n_nodes;
    static_assert(sizeof(spd::Node) == sizeof(sph::BvhNode), "node layout");
    if (c.dtree.nodes) c.s->adopt(c.dtree.nodes, a.n_nodes * sizeof(sph::BvhNode), &d.nodes);
    else {
        std::vector<spd::Node> nodes(a.bvh.nodes.size());
        std::memcpy(nodes.data(), a.bvh.nodes.data(), nodes.size() * sizeof(spd::Node));
        SP_TRY(c.s->upload(nodes, &d.nodes));
    }
    std::vector<float> nrm(h.normals.size() * 3);
    for (size_t i = 0; i < h.normals.size(); ++i) { nrm[3 * i] = h.normals[i].x; nrm[3 * i + 1] = h.normals[i].y; nrm[3 * i + 2] = h.normals[i].z; }
    SP_TRY(c.s->upload(nrm, &d.normals));
    SP_TRY(c.s->upload(h.indices, &d.indices));
    SP_TRY(c.s->upload(h.tri_material, &d.tri_material));
    SP_TRY(c.s->upload(convert_shapes(h), &d.shapes));
    return upload_lights(c.s, a);
}

// The finish's arrays as finish_host made them.  Like run_device_finish it fills wnodes, wslot_tri,
// slot_tri, slot_code and parents, and leaves the wide tree's sizes in s->sizes.
static int upload_finish_host(UploadCall& c)
{
    const HostAccel& a = c.accel;
    spd::Scene&      d = c.s->dev;
    std::vector<uint4> wn(a.wide.words.size() / 4);
    std::memcpy(wn.data(), a.wide.words.data(), a.wide.words.size() * 4);
    SP_TRY(c.s->upload(wn, &d.wnodes));
    SP_TRY(c.s->upload(a.wslot_tri, &d.wslot_tri));
    SP_TRY(c.s->upload(a.slot_tri, &d.slot_tri));
    SP_TRY(c.s->upload(a.slot_code, &d.slot_code));
    SP_TRY(c.s->upload(a.parents, &d.parents));
    c.s->sizes.wide_records = a.wide.words.size() / 20;
    c.s->sizes.wide_slots   = a.wide.slot_of.size();
    c.s->sizes.wide_depth   = a.wide.depth;
    return SP_OK;
}

// The finish on the device (sp_finish.hip): the same arrays from the resident binary tree and the
// resident indices.  The tree's order is build scratch: freed as soon as the finish has read it.
static int run_device_finish(UploadCall& c)
{
    const sph::Scene& h = *c.s->host;
    HostAccel&        a = c.accel;
    spd::Scene&       d = c.s->dev;
    if (c.tm) c.tm->lap(c.tm->ms_copies);
    std::vector<uint32_t> codes(a.part);
    for (size_t i = 0; i < a.part; ++i) codes[i] = code_of(h.prim_kind[a.prims[i]], h.prim_index[a.prims[i]]);
    spf::FinishIn in;
    in.d_nodes      = reinterpret_cast<const sph::BvhNode*>(d.nodes);
    in.n_nodes      = (uint32_t)a.n_nodes;
    in.d_order      = static_cast<const uint32_t*>(c.dtree.order);
    in.h_order      = a.bvh.prim_order.data();
    in.n_slots      = (uint32_t)a.n_slots;
    in.h_codes      = codes.data();
    in.n_prims      = (uint32_t)a.part;
    in.h_verts      = h.vertices.data();
    in.n_verts      = h.vertices.size();
    in.d_indices    = d.indices;
    in.n_indices    = h.indices.size();
    in.want_wide    = a.want_wide;
    in.want_parents = a.walk.stackless;
    spf::FinishOut fo;
    std::string    err;
    const int      rc = spf::finish_device(in, fo, c.timing.fin, err, c.tm != nullptr);
    c.dtree.free_order();
    if (rc != SP_OK) return fail(rc, err);
    c.s->sizes.wide_records = fo.records;
    c.s->sizes.wide_slots   = fo.wide_slots;
    c.s->sizes.wide_depth   = fo.depth;
    c.s->adopt(fo.wnodes, fo.wnodes_bytes, &d.wnodes);
    c.s->adopt(fo.wslot_tri, fo.wslot_tri_bytes, &d.wslot_tri);
    c.s->adopt(fo.slot_tri, fo.slot_tri_bytes, &d.slot_tri);
    c.s->adopt(fo.slot_code, fo.slot_code_bytes, &d.slot_code);
    c.s->adopt(fo.parents, fo.parents_bytes, &d.parents);
    a.walk = walk_plan(c.opts, a.bvh.max_depth, a.lbvh.max_depth, fo.depth);
    if (c.tm) c.tm->lap(c.tm->ms_wide);
    return SP_OK;
}

// ---- image environment lights: the constructor's tables, then the EnvMap records -----------------

// the blocks of a w x h map, each exactly as large as its table; the guide blocks only when asked
static int env_alloc(EnvBlocks& b, const spe::EnvSizes& z, bool guides)
{
    auto need = [](DeviceScratch& d, size_t bytes) -> hipError_t {
        if (d.cap == bytes) return hipSuccess;
        d.reset();
        return bytes ? d.reserve(bytes) : hipSuccess;
    };
    SP_HIP(need(b.radiance, z.texels * sizeof(float4)));
    SP_HIP(need(b.cond_func, z.func * 4));
    SP_HIP(need(b.cond_cdf, z.cdf * 4));
    SP_HIP(need(b.cond_int, z.rows * 4));
    SP_HIP(need(b.marg_func, z.rows * 4));
    SP_HIP(need(b.marg_cdf, z.marg_cdf * 4));
    SP_HIP(need(b.cond_guide, guides ? z.cond_guide * 4 : 0));
    SP_HIP(need(b.marg_guide, guides ? z.marg_guide * 4 : 0));
    return SP_OK;
}

// the record a kernel reads, from the blocks and the image's matrices
static spd::EnvMap env_record(const EnvBlocks& b, const sph::EnvImage& e, const spe::EnvSizes& z, float marg_int)
{
    spd::EnvMap x{};
    x.l2w = e.light_to_world;
    x.w2l = e.world_to_light;
    x.w = e.width; x.h = e.height; x.nu = z.nu; x.nv = z.nv;
    x.radiance   = b.radiance.as<float4>();
    x.cond_func  = b.cond_func.as<float>();
    x.cond_cdf   = b.cond_cdf.as<float>();
    x.cond_int   = b.cond_int.as<float>();
    x.marg_func  = b.marg_func.as<float>();
    x.marg_cdf   = b.marg_cdf.as<float>();
    x.marg_int   = marg_int;
    x.cond_guide = b.cond_guide.as<uint32_t>(); // null: the exact upper_bound replay (identical results)
    x.marg_guide = b.marg_guide.as<uint32_t>();
    x.cond_bits  = z.cond_bits;
    x.marg_bits  = z.marg_bits;
    return x;
}

// Tables of env image i by the host builder (sp_envmap.cpp), copied into its blocks
static int env_build_host(sp_scene* s, size_t i, bool env_guide)
{
    const sph::EnvImage&  e = s->host->env_images[i];
    EnvBlocks&            b = s->env_blocks[i];
    const sph::EnvMap     m = sph::build_env_map(e);
    const spe::EnvSizes   z = spe::env_sizes(e.width, e.height);
    SP_TRY(env_alloc(b, z, m.guided && env_guide));
    std::vector<float4> rad((size_t)m.w * m.h);
    for (size_t k = 0; k < rad.size(); ++k) rad[k] = make_float4(m.radiance[3 * k], m.radiance[3 * k + 1], m.radiance[3 * k + 2], 0.0f);
    auto up = [](DeviceScratch& d, const void* src) { return d.cap ? hipMemcpy(d.ptr, src, d.cap, hipMemcpyHostToDevice) : hipSuccess; };
    SP_HIP(up(b.radiance, rad.data()));
    SP_HIP(up(b.cond_func, m.cond_func.data()));
    SP_HIP(up(b.cond_cdf, m.cond_cdf.data()));
    SP_HIP(up(b.cond_int, m.cond_int.data()));
    SP_HIP(up(b.marg_func, m.marg_func.data()));
    SP_HIP(up(b.marg_cdf, m.marg_cdf.data()));
    SP_HIP(up(b.cond_guide, m.cond_guide.data()));
    SP_HIP(up(b.marg_guide, m.marg_guide.data()));
    b.builder      = SP_ENV_BUILDER_HOST;
    b.guided       = m.guided;
    s->env_recs[i] = env_record(b, e, z, m.marg_int);
    return SP_OK;
}

// The same tables by the device builder (sp_envbuild.hip) from the host's pixels, or from the
// caller's device copy of them
static int env_build_device(sp_scene* s, size_t i, const float* d_pixels, bool env_guide, spe::EnvBuildStats& st, bool timed)
{
    const sph::EnvImage& e = s->host->env_images[i];
    EnvBlocks&           b = s->env_blocks[i];
    const spe::EnvSizes  z = spe::env_sizes(e.width, e.height);
    SP_TRY(env_alloc(b, z, env_guide));
    spe::EnvBuildIn in;
    in.w = e.width; in.h = e.height;
    in.max_radiance = e.max_radiance;
    in.h_pixels     = d_pixels ? nullptr : e.pixels.data();
    in.d_pixels     = d_pixels;
    in.radiance     = b.radiance.as<float4>();
    in.cond_func    = b.cond_func.as<float>();
    in.cond_cdf     = b.cond_cdf.as<float>();
    in.cond_int     = b.cond_int.as<float>();
    in.marg_func    = b.marg_func.as<float>();
    in.marg_cdf     = b.marg_cdf.as<float>();
    in.cond_guide   = b.cond_guide.as<uint32_t>();
    in.marg_guide   = b.marg_guide.as<uint32_t>();
    spe::EnvBuildOut out;
    std::string      err;
    if (const int rc = spe::build_env_device(in, out, st, err, timed)) return fail(rc, err);
    if (!out.guided) { // as the host: one row out of order and the map has no guides
        b.cond_guide.reset();
        b.marg_guide.reset();
    }
    b.builder      = SP_ENV_BUILDER_DEVICE;
    b.guided       = out.guided;
    s->env_recs[i] = env_record(b, e, z, out.marg_int);
    return SP_OK;
}

static int upload_env_records(sp_scene* s) { return s->put(s->env_recs_buf, s->env_recs, &s->dev.envs); }

static int upload_envs(UploadCall& c)
{
    sp_scene* s = c.s;
    s->env_blocks.resize(s->host->env_images.size());
    s->env_recs.resize(s->host->env_images.size());
    for (size_t i = 0; i < s->env_blocks.size(); ++i) {
        spe::EnvBuildStats st;
        SP_TRY(c.hooks.device_env ? env_build_device(s, i, nullptr, c.opts.env_guide, st, false) : env_build_host(s, i, c.opts.env_guide));
    }
    return upload_env_records(s);
}

// RSQRTSS table in its device form (sp_rsqrt_pack.hpp: 16-bit entries where the table allows it)
static int upload_rsqrt_table(UploadCall& c, const sph::RsqrtCapture& rc)
{
    spd::Scene& d = c.s->dev;
    const std::vector<uint32_t> words = spd::rsqrt_device_words(rc.entries.data(), rc.entries.size(), rc.bits, rc.zero_result,
                                                                rc.denorm_result, c.hooks.rsqrt_pack);
    const int      rs_shift = (int)words[3];
    const uint32_t rs_hi    = words[4];
    SP_TRY(c.s->upload(words, &d.rsqrt_entries));
    d.rsqrt_shift  = rs_shift;
    d.rsqrt_hi     = rs_shift ? rs_hi : 0u;
    d.rsqrt_bits   = rc.bits;
    d.rsqrt_zero   = rc.zero_result;
    d.rsqrt_denorm = rc.denorm_result;
    return SP_OK;
}

static void apply_walk_plan(sp_scene* s, const UploadOpts& opts, const WalkPlan& w)
{
    spd::Scene&     d = s->dev;
    d.ordered         = opts.bvh_mode == 1 ? 0 : 1; // reference order is part of the bit-exact contract
    d.wide_closest    = w.wide_closest ? 1 : 0;
    d.stackless       = w.stackless ? 1 : 0;
    d.stack_depth     = w.stack_depth;
    d.stack_words     = w.stack_words;
    d.any_stack_words = w.any_stack_words;
    d.merge_queries   = 1; // per render: SP_RENDER_PER_LANE_QUERIES clears it
}

// what every render call expects to find (the rest of RenderScratch grows on demand)
static int create_render_handles(sp_scene* s)
{
    RenderScratch& r = s->scratch;
    SP_HIP(r.tile_counter.reserve(sizeof(int32_t)));
    SP_HIP(r.counters.reserve(8 * sizeof(unsigned long long)));
    SP_HIP(hipEventCreate(&r.ev0[0]));
    SP_HIP(hipEventCreate(&r.ev1[0]));
    SP_HIP(hipEventCreateWithFlags(&r.ev_done[0], hipEventDisableTiming));
    for (hipEvent_t& e : r.ev_tiles.h) SP_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (hipEvent_t& e : r.ev_cams.h) SP_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return SP_OK;
}

static void print_upload_timing(const UploadCall& c)
{
    const UploadTiming&     t = *c.tm;
    const spb::BuildStats&  b = t.dev;
    const spb::SahStats&    q = t.sah;
    const spf::FinishStats& f = t.fin;
    std::fprintf(stderr,
                 "sp_upload_timing {\"builder\": \"%s\", \"bvh_mode\": %d, \"prims\": %zu, \"nodes\": %zu, \"depth\": %d, "
                 "\"stackless\": %d, \"bounds_ms\": %.3f, \"bvh_ms\": %.3f, \"wide_ms\": %.3f, \"pack_ms\": %.3f, \"copies_ms\": %.3f, "
                 "\"device\": {\"bounds_up_ms\": %.3f, \"codes_ms\": %.3f, \"sort_ms\": %.3f, \"hierarchy_ms\": %.3f, \"fit_ms\": %.3f, "
                 "\"copy_back_ms\": %.3f, \"passes\": %d, \"peak_scratch_bytes\": %zu}, "
                 "\"device_sah\": {\"bounds_up_ms\": %.3f, \"levels_ms\": %.3f, \"subtrees_ms\": %.3f, \"number_ms\": %.3f, "
                 "\"emit_ms\": %.3f, \"copy_back_ms\": %.3f, \"levels\": %d, \"level_nodes\": %u, \"subtrees\": %u, "
                 "\"peak_scratch_bytes\": %zu}, "
                 "\"finish\": \"%s\", \"device_finish\": {\"inputs_up_ms\": %.3f, \"collapse_ms\": %.3f, \"sums_ms\": %.3f, "
                 "\"bases_ms\": %.3f, \"emit_ms\": %.3f, \"pack_ms\": %.3f, \"parents_ms\": %.3f, \"levels\": %d, "
                 "\"peak_scratch_bytes\": %zu}}\n",
                 c.opts.builder == SP_BUILDER_DEVICE ? "device" : (c.opts.builder == SP_BUILDER_DEVICE_SAH ? "device_sah" : "host"), c.opts.bvh_mode, c.accel.n_slots, c.accel.n_nodes,
                 c.accel.bvh.max_depth, c.s->dev.stackless, t.ms_bounds, t.ms_bvh, t.ms_wide, t.ms_pack, t.ms_copies, b.ms_bounds_up,
                 b.ms_codes, b.ms_sort, b.ms_hierarchy, b.ms_fit, b.ms_copy_back, b.passes, b.peak_bytes, q.ms_bounds_up, q.ms_levels,
                 q.ms_subtrees, q.ms_number, q.ms_emit, q.ms_copy_back, q.levels, q.top_nodes, q.subtrees, q.peak_bytes,
                 c.device_finish() ? "device" : "host", f.ms_inputs_up, f.ms_collapse, f.ms_sums, f.ms_bases, f.ms_emit, f.ms_pack,
                 f.ms_parents, f.levels, f.peak_bytes);
}

// Everything after the arguments; `device` and `opts`, which make the scene resident, are set last
static int build_residency(UploadCall& c)
{
    sp_scene*         s = c.s;
    const sph::Scene& h = *s->host;
    HostAccel&        a = c.accel;
    SP_HIP(hipSetDevice(c.device));
    const auto& rc = sph::rsqrt_active();
    if (rc.entries.empty()) return fail(SP_ERR_UNSUPPORTED, "RSQRTSS table capture failed");
    if (!rc.verified) return fail(SP_ERR_UNSUPPORTED, "RSQRTSS table could not be verified on this host CPU");
    std::vector<spd::Material> mats;
    SP_TRY(convert_materials(h, mats));
    c.timing = UploadTiming{}; // the stage times start here
    build_trees(h, a, c.opts, BuildOn::DEVICE, c.tm, c.device_finish() ? &c.dtree : nullptr, c.hooks.sah_small);
    std::vector<sph::PrimBounds>().swap(a.bounds); // nothing below reads them: not held beside the records
    if (!c.device_finish()) finish_host(h, a, c.opts, c.tm);
    SP_TRY(upload_scene_arrays(c));
    SP_TRY(c.device_finish() ? run_device_finish(c) : upload_finish_host(c));
    SP_TRY(upload_envs(c));
    SP_TRY(s->upload(mats, &s->dev.materials));
    SP_TRY(upload_rsqrt_table(c, rc));
    s->sizes.geom_depth  = a.bvh.max_depth;
    s->sizes.light_depth = a.lbvh.max_depth;
    s->sizes.geom_nodes  = a.n_nodes;
    s->sizes.geom_slots  = a.n_slots;
    apply_walk_plan(s, c.opts, a.walk);
    SP_TRY(create_render_handles(s));
    if (c.tm) {
        c.tm->lap(c.tm->ms_copies);
        print_upload_timing(c);
    }
    s->opts   = c.opts;
    s->device = c.device;
    return SP_OK;
}

// No C++ exception crosses the C ABI: host-side failures (allocation, BVH encoding limits) come
// back as error codes with sp_last_error() set.  Refused arguments leave the scene as it was; a
// build that fails half way, by code or by exception, leaves no resident scene.
int sp_scene_upload_with(sp_scene* s, int32_t device, const sp_upload_params* params, const sp_build_params* build)
{
    if (!s) return fail(SP_ERR_ARG, "null scene");
    std::lock_guard<std::mutex> lock(s->mu);
    bool building = false;
    int  rc       = SP_OK;
    try {
        UploadCall c{ s, device, UploadHooks::from_env() };
        bool       resident = false;
        SP_TRY(validate_upload(c, params, build, resident));
        if (resident) return SP_OK;
        if (c.hooks.timing) c.tm = &c.timing;
        building = true;
        s->release();
        ++s->generation;
        rc = build_residency(c);
    } catch (const sph::SpError& e) {
        rc = fail(e.code, e.what());
    } catch (const std::exception& e) {
        rc = fail(SP_ERR_UNSUPPORTED, std::string("scene upload failed: ") + e.what());
    }
    if (rc != SP_OK && building) s->release();
    return rc;
}
#undef SP_TRY

int sp_scene_upload_ex(sp_scene* s, int32_t device, const sp_upload_params* params)
{
    return sp_scene_upload_with(s, device, params, nullptr);
}

int sp_scene_upload(sp_scene* s, int32_t device, int32_t bvh_mode)
{
    sp_upload_params p{};
    p.bvh_mode = bvh_mode;
    return sp_scene_upload_ex(s, device, &p);
}

static int render_tiles_impl(sp_scene* s, const sp_render_params* p, float* d_out, sp_render_stats* stats);
int sp_render_tiles(sp_scene* s, const sp_render_params* p, float* d_out, sp_render_stats* stats)
{
    if (!s) return fail(SP_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lock(s->mu); // calls on one scene run one at a time (sp_scene::mu)
    try {
        return render_tiles_impl(s, p, d_out, stats);
    } catch (const sph::SpError& e) {
        return fail(e.code, e.what());
    } catch (const std::exception& e) {
        return fail(SP_ERR_HIP, std::string("render failed: ") + e.what());
    }
}

using splan::ChunkPlan;
using splan::RenderHooks;

// ---- a request, resolved (sp_render_tiles, sp_render_tiles_host, sp_progress_create) -------------

// The integrator: NOT_SPECIFIED falls back to the scene's, then to DirectLighting.  The megakernel
// occupancy request with it: DirectLighting 1..4 waves per SIMD, IterativeRRNEE 2..4; the other
// integrators have one variant each (0 = automatic)
static int resolve_integrator(const sp_scene* s, int32_t requested, int waves_req, int32_t& integ)
{
    integ = requested;
    if (integ == SP_INTEGRATOR_NOT_SPECIFIED) integ = s->host->integrator;
    if (integ == SP_INTEGRATOR_NOT_SPECIFIED) integ = SP_INTEGRATOR_DIRECT_LIGHTING; // main.cpp:390
    if (integ < SP_INTEGRATOR_MANDELBROT || integ > SP_INTEGRATOR_WHITTED) return fail(SP_ERR_ARG, "Unknown integrator type");
    if (waves_req != 0) {
        const bool ok = integ == SP_INTEGRATOR_DIRECT_LIGHTING ? (waves_req >= 1 && waves_req <= 4)
                        : integ == SP_INTEGRATOR_ITERATIVE_RRNEE ? (waves_req >= 2 && waves_req <= 4)
                                                                  : false;
        if (!ok) return fail(SP_ERR_ARG, "waves_per_simd: DirectLighting 1-4, IterativeRRNEE 2-4, else 0");
    }
    return SP_OK;
}

// The tiles: num_tiles entries of either list, or every tile of the frame
struct TileList {
    bool    listed = false;
    int64_t n = 0, total = 0;
};
static TileList tile_list(const sp_scene* s, const int32_t* ids, const int32_t* d_ids, int64_t num_tiles)
{
    TileList t;
    sp_tile_count(s->dev.width, s->dev.height, &t.total);
    t.listed = ids || d_ids;
    t.n      = t.listed ? num_tiles : t.total;
    return t;
}
static int check_tile_list(const TileList& t, const int32_t* ids)
{
    if (t.n < 0) return fail(SP_ERR_ARG, "num_tiles < 0");
    if (ids)
        for (int64_t i = 0; i < t.n; ++i)
            if (ids[i] < 0 || ids[i] >= t.total) return fail(SP_ERR_ARG, "tile id out of range");
    return SP_OK;
}

static int device_cus(sp_scene* s)
{
    if (s->scratch.n_cu == 0) {
        hipDeviceProp_t prop;
        SP_HIP(hipGetDeviceProperties(&prop, s->device));
        s->scratch.n_cu = prop.multiProcessorCount;
    }
    return SP_OK;
}

// dynamic LDS of a shading block: the RSQRTSS table and its four waves' traversal stacks
static size_t shading_lds(const spd::Scene& d) { return (size_t)spd::rsqrt_words(d) * 4 + (size_t)4 * d.stack_words * 64 * 4; }

// ---- the megakernel's launch setup (sp_render_tiles and calls on progress objects) --------------

struct MegaSetup {
    spd::MegaFamily family = spd::MegaFamily::Render;
    int             integ = 0, variant = 0, blocks = 0;
    size_t          lds_bytes = 0; // dynamic
    size_t          waves = 0;     // persistent waves of the launch (4 per block)
    spd::Scene      sc_run{};      // the resident scene with this render's options
    spd::RenderArgs a{};           // all but out and spp
};

// Occupancy variant, persistent blocks, the generator store and the deep-recursion buffer (both in
// the scene's scratch), and the launch arguments every kernel of the family takes.
static int mega_setup(sp_scene* s, spd::MegaFamily family, int integ, int waves_req, const int32_t* d_ids, int64_t n_tiles,
                      MegaSetup& m)
{
    RenderScratch& r = s->scratch;
    m.family    = family;
    m.integ     = integ;
    m.lds_bytes = shading_lds(s->dev);
    // the kernel's static LDS counts too (the largest over the variants this call may pick)
    size_t lds_static = 0;
    for (int v = 2; v <= 4; ++v) lds_static = std::max(lds_static, spd::kernel_static_lds(spd::mega_kernel(family, integ, v)));
    const size_t lds_all = m.lds_bytes + lds_static;
    if (lds_all > 160 * 1024) return fail(SP_ERR_UNSUPPORTED, "BVH too deep for the LDS traversal stack");
    // waves per SIMD the kernel is compiled for (SP_KERNEL_VARIANT): DirectLighting 4,
    // IterativeRRNEE 3 -- but never more than the LDS lets run (one 4-wave block per wave per
    // SIMD): a deep BVH's stacks (lucy: 3 blocks per CU) would leave the extra occupancy's
    // register budget paid for in spills and unused (lucy 1080p @ 256 spp: 2007 Mrays/s at 3
    // waves, 1879 at 4; profiles/r02/s5)
    const int lds_waves = (int)std::min<size_t>(8, (160 * 1024) / lds_all);
    m.variant           = integ == SP_INTEGRATOR_ITERATIVE_RRNEE ? 3 : 4;
    m.variant           = std::max(2, std::min(m.variant, lds_waves));
    if (waves_req) m.variant = waves_req;
    const int per_cu = spd::kernel_blocks_per_cu(spd::mega_kernel(family, integ, m.variant), m.lds_bytes);
    m.blocks         = (int)std::max<int64_t>(1, std::min((int64_t)r.n_cu * per_cu, (n_tiles + 3) / 4));
    m.waves          = (size_t)m.blocks * 4;
    SP_HIP(r.mt_state.reserve(m.waves * 2 * (size_t)spd::MT_GEN_WORDS * sizeof(uint64_t)));
    m.sc_run         = s->dev;
    m.a              = spd::RenderArgs{};
    m.a.tile_ids     = d_ids;
    m.a.num_tiles    = n_tiles;
    m.a.tiles_x      = (s->dev.width + 7) / 8;
    m.a.integrator   = integ;
    m.a.tile_counter = r.tile_counter.as<int32_t>();
    m.a.mt_state     = r.mt_state.as<uint64_t>();
    m.a.counters     = r.counters.as<unsigned long long>();
    // BruteForce / Whitted recursion deeper than the in-register arrays: global level records
    if ((integ == SP_INTEGRATOR_BRUTE_FORCE || integ == SP_INTEGRATOR_WHITTED) && s->dev.max_depth > MAX_RECURSION) {
        const size_t lanes = m.waves * 64;
        SP_HIP(r.deep_buf.reserve(lanes * ((size_t)s->dev.max_depth + 1) * 5 * sizeof(float)));
        m.a.deep        = r.deep_buf.as<float>();
        m.a.deep_stride = lanes;
    }
    return SP_OK;
}

// Tile order (sp_mega.hip tile_order): a one-sample probe pass times every tile into tile_time, and
// the queue order is written to `order` (the scene's scratch, or a progress object's own arrays).
// Part of the render (timed with it); stream-ordered, no host wait.  Leaves the queue head at zero.
static int order_tiles(sp_scene* s, const MegaSetup& m, float* probe_out, float* tile_time, int32_t* order, float hoist,
                       int probe_step, int neighbours, hipStream_t stream)
{
    RenderScratch& r = s->scratch;
    SP_HIP(r.probe_counters.reserve(8 * sizeof(unsigned long long)));
    spd::RenderArgs pr = m.a;
    pr.out        = probe_out;
    pr.spp        = 1; // 2 or 4 probe samples measured no better (profiles/r03/ab_tile_order.txt, r04/tile_classes)
    pr.tile_time  = tile_time;
    pr.counters   = r.probe_counters.as<unsigned long long>(); // the probe's rays are not the render's
    pr.tile_diag  = nullptr;
    pr.probe_step = probe_step;
    SP_HIP(spd::launch_probe(m.sc_run, pr, m.integ, m.variant, m.blocks, m.lds_bytes, stream));
    SP_HIP(spd::launch_tile_order(tile_time, m.a.num_tiles, hoist, neighbours, probe_step, order, stream));
    SP_HIP(hipMemsetAsync(r.tile_counter.ptr, 0, sizeof(int32_t), stream));
    return SP_OK;
}

// The end of every call on a scene's scratch: ev1 closes the timed span, ev_done orders the next call
static int end_call(sp_scene* s, hipStream_t stream)
{
    RenderScratch& r = s->scratch;
    SP_HIP(hipEventRecord(r.ev1, stream));
    SP_HIP(hipEventRecord(r.ev_done, stream));
    r.done_rec = true;
    return SP_OK;
}

// the host waits for the last call queued on the scene's scratch
static int wait_done(sp_scene* s)
{
    if (s->scratch.done_rec) SP_HIP(hipEventSynchronize(s->scratch.ev_done));
    return SP_OK;
}

// Waits for the call (ev1) and fills the statistics every call reports; c: the device counters
static int read_stats(sp_scene* s, int pipeline, int launches, sp_render_stats* stats, unsigned long long (&c)[8])
{
    RenderScratch& r = s->scratch;
    SP_HIP(hipEventSynchronize(r.ev1));
    SP_HIP(hipMemcpy(c, r.counters.ptr, sizeof(c), hipMemcpyDeviceToHost));
    float ms = 0.0f;
    SP_HIP(hipEventElapsedTime(&ms, r.ev0, r.ev1));
    stats->rays        = c[0];
    stats->shadow_rays = c[1];
    stats->samples     = c[2];
    stats->rng_draws   = c[3];
    stats->kernel_ms   = ms;
    stats->pipeline    = pipeline;
    stats->launches    = launches;
    stats->parts       = 1;
    stats->stack_depth = s->dev.stack_depth;
    return SP_OK;
}

// ---- sp_render_tiles ------------------------------------------------------------------------------

// One call, resolved: what its steps share and what they report
struct RenderCall {
    sp_scene*               s;
    const sp_render_params* p;
    float*                  d_out;
    hipStream_t             stream;
    RenderHooks             hooks;
    int32_t                 integ = 0;
    TileList                tiles;
    const int32_t*          d_ids = nullptr; // device tile list (nullptr: slot = tile)
    bool                    timing = false;
    double                  ck_max_gb = 0.0; // the caller's cap on the chunk and tail buffers
    size_t                  free_b = 0;      // free device memory at the top of the call
    double                  ck_budget = 0.0;
    bool                    image_light = false;
    splan::Plan             plan;
    // for the statistics
    int     launches = 0, parts_used = 1;
    int64_t tail_k = 0; // megakernel tail chunks: tiles cut (tail_ch chunks each)
    int     tail_ch = 0;
    float   stage[4] = { 0, 0, 0, 0 };
};

static int validate_render(const sp_scene* s, const sp_render_params* p, const float* d_out)
{
    if (!s || !p || !d_out) return fail(SP_ERR_ARG, "null argument");
    if (s->device < 0) return fail(SP_ERR_STATE, "sp_scene_upload must be called before sp_render_tiles");
    if (p->samples_per_pixel == 0) return fail(SP_ERR_ARG, "samples_per_pixel must be > 0");
    if (p->reserved != 0) return fail(SP_ERR_ARG, "sp_render_params.reserved must be 0");
    if (!(p->tail_fraction <= 1.0f)) return fail(SP_ERR_ARG, "tail_fraction must be at most 1 (and not NaN)");
    if (p->tile_ids && p->d_tile_ids) return fail(SP_ERR_ARG, "give tile_ids (host) or d_tile_ids (device), not both");
    if (p->chunks_per_pixel < 0) return fail(SP_ERR_ARG, "chunks_per_pixel < 0");
    if (!(p->chunk_max_gb >= 0.0f)) return fail(SP_ERR_ARG, "chunk_max_gb < 0");
    if (p->tile_order_factor != p->tile_order_factor) return fail(SP_ERR_ARG, "tile_order_factor is NaN");
    if ((p->flags & ~(3 | SP_RENDER_STAGE_TIMING | SP_RENDER_PER_LANE_QUERIES)) != 0) return fail(SP_ERR_ARG, "unknown flags");
    return SP_OK;
}

// A host tile list goes to the device through the next pinned buffer of the ring, so the caller's
// array is free once the call returns; the host waits only if that buffer's copy (STAGE_RING calls
// back) has not run
static int stage_ids(sp_scene* s, const int32_t* ids, int64_t n, hipStream_t stream, const int32_t*& d_ids)
{
    RenderScratch& r     = s->scratch;
    const size_t   bytes = (size_t)n * sizeof(int32_t);
    SP_HIP(r.d_tiles.reserve(bytes));
    const int k  = r.stage_next;
    r.stage_next = (k + 1) % RenderScratch::STAGE_RING;
    if (r.tiles_rec[k]) SP_HIP(hipEventSynchronize(r.ev_tiles[k]));
    SP_HIP(r.h_tiles[k].reserve(bytes));
    std::memcpy(r.h_tiles[k].ptr, ids, bytes);
    SP_HIP(hipMemcpyAsync(r.d_tiles.ptr, r.h_tiles[k].ptr, bytes, hipMemcpyHostToDevice, stream));
    SP_HIP(hipEventRecord(r.ev_tiles[k], stream));
    r.tiles_rec[k] = true;
    d_ids          = r.d_tiles.as<int32_t>();
    return SP_OK;
}
static int stage_tile_list(RenderCall& c) { return stage_ids(c.s, c.p->tile_ids, c.tiles.n, c.stream, c.d_ids); }

// Which pipeline (sp_plan.hpp plan_render), and the sample chunks' buffers when it is theirs
static int plan_call(RenderCall& c)
{
    sp_scene*      s = c.s;
    RenderScratch& r = s->scratch;
    const int asked  = c.p->flags & 3;
    if (asked == SP_PIPELINE_SAMPLE_CHUNKS && c.integ != SP_INTEGRATOR_DIRECT_LIGHTING)
        return fail(SP_ERR_UNSUPPORTED, "the sample-chunk pipeline implements DirectLighting");
    if (asked == SP_PIPELINE_WAVEFRONT && !splan::wave_ok(c.integ, s->dev.n_lights))
        return fail(SP_ERR_UNSUPPORTED, "the wavefront pipeline implements DirectLighting (<= 32 lights)");
    c.ck_max_gb = c.p->chunk_max_gb > 0.0f ? (double)c.p->chunk_max_gb : c.hooks.chunk_max_gb;
    // budget: the caller's cap, and never more than the device can still give (the buffer held
    // from an earlier call is freed first)
    size_t total_b = 0;
    SP_HIP(hipMemGetInfo(&c.free_b, &total_b));
    c.ck_budget = std::min(c.ck_max_gb * 1e9, (double)c.free_b + (double)r.ck_buf.cap);
    for (const auto& l : s->host->lights) c.image_light = c.image_light || l.kind == SP_LIGHT_IMAGE_ENVIRONMENT;
    splan::PlanIn in;
    in.integ         = c.integ;
    in.n_tiles       = c.tiles.n;
    in.spp           = c.p->samples_per_pixel;
    in.n_lights      = s->dev.n_lights;
    in.image_light   = c.image_light;
    in.n_cu          = r.n_cu;
    in.tail_fraction = c.p->tail_fraction;
    in.chunks_req    = c.p->chunks_per_pixel;
    in.ck_budget     = c.ck_budget;
    in.asked         = asked;
    c.plan           = splan::plan_render(in, c.hooks);
    if (c.plan.pipeline == SP_PIPELINE_SAMPLE_CHUNKS && c.plan.cp.total > r.ck_buf.cap) {
        if ((double)c.plan.cp.total > c.ck_budget)
            return fail(SP_ERR_UNSUPPORTED, "sample-chunk pipeline: buffers exceed the budget (chunk_max_gb / free "
                                            "device memory; render fewer tiles per call)");
        const hipError_t e = r.ck_buf.reserve(c.plan.cp.total);
        if (e != hipSuccess) {
            if (asked != SP_PIPELINE_AUTO) return fail(SP_ERR_HIP, std::string("sample-chunk buffers: ") + hipGetErrorString(e));
            c.plan.pipeline = SP_PIPELINE_MEGAKERNEL; // AUTO: the megakernel needs no per-sample buffers
        }
    }
    return SP_OK;
}

static int run_wavefront(RenderCall& c)
{
    sp_scene*      s = c.s;
    RenderScratch& r = s->scratch;
    const int64_t  n_tiles = c.tiles.n;
    const size_t stack_lds = (size_t)4 * s->dev.stack_words * 64 * 4;
    if (stack_lds > 160 * 1024) return fail(SP_ERR_UNSUPPORTED, "BVH too deep for the LDS traversal stack");
    // Pixels in flight per pass: all requested tiles unless the state would exceed the budget
    // (SP_WAVE_MAX_GB, default 64 GB of the 288 GB HBM); larger jobs run in tile chunks.
    const size_t  per_pix   = spd::wave_bytes_per_pixel(s->dev.n_lights);
    // queue items pack the pixel slot in 27 bits (sp_wave.hip wf_shade)
    const int64_t max_tiles = std::min<int64_t>((int64_t)1 << 21,
                                                std::max<int64_t>(1, (int64_t)(c.hooks.wave_max_gb * 1e9 / (double)(per_pix * 64))));
    const int64_t chunk     = std::min<int64_t>(n_tiles, max_tiles);
    const size_t  n         = (size_t)chunk * 64;
    const size_t  need      = n * per_pix + spd::wave_stat_bytes((int64_t)n) + spd::wave_queue_bytes((int64_t)n, s->dev.n_lights) +
                              n * (size_t)std::max(1, s->dev.n_lights) + 256 * 12;
    SP_HIP(r.wave_buf.reserve(need));
    // carve: every array 256-byte aligned (n is a multiple of 64)
    char* b    = r.wave_buf.as<char>();
    auto  take = [&](size_t bytes) { char* p = b; b += (bytes + 255) & ~(size_t)255; return p; };
    spd::WaveArgs w{};
    w.n        = (int64_t)n;
    w.tiles_x  = (s->dev.width + 7) / 8;
    w.spp      = c.p->samples_per_pixel;
    w.mt_state = reinterpret_cast<uint64_t*>(take(n / 64 * 2 * spd::MT_GEN_WORDS * 8));
    w.sh       = reinterpret_cast<float4*>(take(n * (size_t)std::max(1, s->dev.n_lights) * 32));
    w.hit      = reinterpret_cast<float4*>(take(n * 16));
    w.shp      = reinterpret_cast<float4*>(take(n * 16));
    w.acc      = reinterpret_cast<float*>(take(n * 12));
    w.rstate   = reinterpret_cast<uint32_t*>(take(n * 4));
    w.queue    = reinterpret_cast<uint32_t*>(take(spd::wave_queue_bytes((int64_t)n, s->dev.n_lights)));
    w.qcount   = nullptr; // per part (wave_render)
    w.vis      = reinterpret_cast<uint8_t*>(take(n * (size_t)std::max(1, s->dev.n_lights)));
    w.wstat    = reinterpret_cast<unsigned long long*>(take(spd::wave_stat_bytes((int64_t)n)));
    w.counters = r.counters.as<unsigned long long>();
    // SP_WAVE_DIAG=<file>: per-wave timeline of one sample's primary + shadow launches
    DeviceScratch diag;
    const size_t  diag_n = 2 * (n / 64) * 4;
    if (c.hooks.wave_diag) {
        SP_HIP(diag.reserve(diag_n * 8));
        SP_HIP(hipMemsetAsync(diag.ptr, 0, diag_n * 8, c.stream));
    }
    w.diag = diag.as<unsigned long long>();
    const int per_cu = spd::wave_traverse_blocks_per_cu(s->dev);
    // two halves of the tile list on two streams, their shading kernels alternating (+11 %;
    // 3 or 4 parts measured 1988 / 1821 against 2068 Mrays/s)
    const int n_parts = std::min(2, spd::WF_MAX_PARTS);
    if (!r.ev_fork) {
        SP_HIP(hipEventCreateWithFlags(&r.ev_fork[0], hipEventDisableTiming));
        for (auto& e : r.ev_shade.h) SP_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    for (int k = 0; k + 1 < n_parts; ++k)
        if (!r.aux_stream[k]) {
            SP_HIP(hipStreamCreateWithFlags(&r.aux_stream[k], hipStreamNonBlocking));
            SP_HIP(hipEventCreateWithFlags(&r.ev_join[k], hipEventDisableTiming));
        }
    std::vector<hipEvent_t>& stage_ev = r.stage_ev.v;
    const size_t             n_ev     = c.timing ? 3 * (size_t)w.spp + 3 : 0;
    while (stage_ev.size() < n_ev) {
        hipEvent_t e;
        SP_HIP(hipEventCreate(&e));
        stage_ev.push_back(e);
    }
    SP_HIP(hipEventRecord(r.ev0, c.stream));
    for (int64_t t0 = 0; t0 < n_tiles; t0 += chunk) {
        const int64_t nt = std::min<int64_t>(chunk, n_tiles - t0);
        w.n        = nt * 64;
        w.tile_ids = c.d_ids ? c.d_ids + t0 : nullptr;
        if (!c.d_ids && t0 > 0) {
            // identity ids beyond the first chunk: materialise them
            std::vector<int32_t> ids((size_t)nt);
            for (int64_t i = 0; i < nt; ++i) ids[(size_t)i] = (int32_t)(t0 + i);
            SP_HIP(r.d_tiles.reserve((size_t)chunk * sizeof(int32_t)));
            SP_HIP(hipMemcpyAsync(r.d_tiles.ptr, ids.data(), (size_t)nt * 4, hipMemcpyHostToDevice, c.stream));
            SP_HIP(hipStreamSynchronize(c.stream));
            w.tile_ids = r.d_tiles.as<int32_t>();
        }
        w.pb = 0;
        w.pe = w.n;
        SP_HIP(spd::wave_render(s->dev, w, c.d_out + (size_t)t0 * 64 * 3, per_cu, r.n_cu, c.stream,
                                c.timing ? stage_ev.data() : nullptr, r.aux_stream.h, n_parts - 1, r.ev_fork, r.ev_join.h,
                                r.ev_shade.h, &c.parts_used));
        c.launches += 3 + 4 * (int)w.spp;
        if (w.diag) {
            std::vector<unsigned long long> h(diag_n);
            SP_HIP(hipStreamSynchronize(c.stream));
            SP_HIP(hipMemcpy(h.data(), diag.ptr, diag_n * 8, hipMemcpyDeviceToHost));
            if (FILE* f = std::fopen(c.hooks.wave_diag, "wb")) {
                std::fwrite(h.data(), 8, diag_n, f);
                std::fclose(f);
            }
            diag.reset();
            w.diag = nullptr;
        }
        if (c.timing) {
            SP_HIP(hipEventSynchronize(stage_ev[n_ev - 1]));
            auto el = [&](size_t a, size_t b) {
                float ms = 0.0f;
                (void)hipEventElapsedTime(&ms, stage_ev[a], stage_ev[b]);
                return ms;
            };
            c.stage[0] += el(0, 1) + el(n_ev - 2, n_ev - 1);
            for (uint32_t i = 0; i < w.spp; ++i) {
                const size_t b = 1 + 3 * (size_t)i;
                c.stage[1] += el(b, b + 1);
                c.stage[2] += el(b + 1, b + 2);
                c.stage[3] += el(b + 2, b + 3);
            }
        }
    }
    return SP_OK;
}

// sp_chunk.hip: camera rays for all (pixel, sample) at once, a per-pixel replay of the stream
// positions into the generator store, then every (tile, chunk) shaded in parallel, and the
// in-order sum (buffers: splan::chunk_plan, reserved by plan_call)
static int run_chunks(RenderCall& c)
{
    sp_scene*        s  = c.s;
    RenderScratch&   r  = s->scratch;
    const ChunkPlan& cp = c.plan.cp;
    const int64_t    n_tiles = c.tiles.n;
    const uint32_t   spp_u   = c.p->samples_per_pixel;
    const size_t lds_bytes = shading_lds(s->dev);
    if (lds_bytes > 160 * 1024) return fail(SP_ERR_UNSUPPORTED, "BVH too deep for the LDS traversal stack");
    const size_t n_px   = (size_t)n_tiles * 64;
    SP_HIP(r.ck_ctr.reserve(2 * sizeof(int32_t)));
    const int per_cu = spd::chunk_blocks_per_cu(lds_bytes);
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)r.n_cu * per_cu, (n_tiles * cp.chunks + 3) / 4));
    char*          base = r.ck_buf.as<char>();
    spd::ChunkArgs a{};
    a.tile_ids    = c.d_ids;
    a.num_tiles   = n_tiles;
    a.tiles_x     = (s->dev.width + 7) / 8;
    a.spp         = spp_u;
    a.chunks      = (uint32_t)cp.chunks;
    a.chunk_len   = cp.len;
    a.n_px        = n_px;
    a.hits        = reinterpret_cast<float4*>(base);
    a.L           = reinterpret_cast<float*>(base + cp.b_hits);
    a.gens        = reinterpret_cast<uint64_t*>(base + cp.b_hits + cp.b_L);
    a.gens_per_px = cp.gens;
    a.snap_ctl    = reinterpret_cast<uint32_t*>(base + cp.b_hits + cp.b_L + cp.b_snap);
    a.draws       = cp.known_draws ? reinterpret_cast<uint16_t*>(base + cp.b_hits + cp.b_L + cp.b_snap + cp.b_ctl) : nullptr;
    a.n_lights    = s->dev.n_lights;
    a.counter     = r.ck_ctr.as<int32_t>();
    a.counters    = r.counters.as<unsigned long long>();
    a.out         = c.d_out;
    // Fused form (known draw counts): ck_camera, then the counts and the shading in ONE persistent
    // queue of the megakernel's tail kernel (sp_mega.hpp, RenderArgs::tail_front): each tile's
    // prep (stream positions, generations into the store) runs P tiles ahead of its chunks, so the
    // HBM-bound twists overlap the shading instead of running as a phase of their own (ck_count).
    // Same store contents and chunk starts, same image.  SP_CK_FUSED=0: the four-kernel form.
    bool fused = cp.known_draws && c.hooks.ck_fused;
    SP_HIP(hipMemsetAsync(r.ck_ctr.ptr, 0, 2 * sizeof(int32_t), c.stream));
    // the tail kernel's LDS (the megakernel's: RSQRTSS table + per-wave stacks) and occupancy
    if (fused && lds_bytes + spd::kernel_static_lds(spd::mega_kernel(spd::MegaFamily::Render, SP_INTEGRATOR_DIRECT_LIGHTING, 4)) > 160 * 1024)
        fused = false;
    if (!fused) {
        SP_HIP(hipEventRecord(r.ev0, c.stream));
        SP_HIP(spd::chunk_render(s->dev, a, blocks, r.n_cu, c.stream));
        c.launches = 4;
        return SP_OK;
    }
    const size_t a_hdr = 256, a_rdy = ((size_t)n_tiles * 4 + 255) / 256 * 256;
    SP_HIP(r.tail_buf.reserve(a_hdr + 2 * a_rdy));
    char*         tb = r.tail_buf.as<char>();
    spd::TailArgs ta{};
    ta.n_prep      = n_tiles;
    ta.n_items     = n_tiles * cp.chunks;
    ta.chunks      = (uint32_t)cp.chunks;
    ta.chunk_len   = cp.len;
    ta.gens_per_px = cp.gens;
    ta.n_px        = n_px;
    ta.hits        = a.hits;
    ta.L           = a.L;
    ta.gens        = a.gens;
    ta.snap_ctl    = a.snap_ctl;
    ta.draws       = a.draws;
    ta.ready       = reinterpret_cast<uint32_t*>(tb + a_hdr);
    // the camera pass as the queue's first items (SP_CK_CAMFOLD; blocks of SP_CK_CAM_BLOCK
    // samples per item) instead of the ck_camera kernel before it
    const bool cam_fold = c.hooks.ck_camfold;
    if (cam_fold) {
        ta.cam_block = c.hooks.ck_cam_block;
        ta.n_cam     = n_tiles * (int64_t)((spp_u + ta.cam_block - 1) / ta.cam_block);
        ta.cam_done  = reinterpret_cast<uint32_t*>(tb + a_hdr + a_rdy);
        ta.draws_out = a.draws;
    }
    SP_HIP(hipMemcpyAsync(tb, &ta, sizeof(ta), hipMemcpyHostToDevice, c.stream));
    SP_HIP(hipMemsetAsync(ta.ready, 0, 2 * a_rdy, c.stream));
    spd::RenderArgs ra{};
    ra.out          = c.d_out;
    ra.tile_ids     = c.d_ids;
    ra.num_tiles    = n_tiles;
    ra.tiles_x      = a.tiles_x;
    ra.spp          = spp_u;
    ra.integrator   = c.integ;
    ra.tile_counter = r.ck_ctr.as<int32_t>();
    ra.counters     = r.counters.as<unsigned long long>();
    ra.tail_prep    = ta.n_prep;
    ra.tail_items   = ta.n_items;
    const int     t_per_cu = spd::kernel_blocks_per_cu(spd::tail_kernel(0), lds_bytes); // 0: sp_fused_kernel
    const int64_t t_waves  = (int64_t)r.n_cu * t_per_cu * 4;
    // P: the preps ahead of the first chunks; the rest are dealt one per tile's chunks
    ra.tail_front = std::max<int64_t>(1, t_waves / c.hooks.ck_front_div);
    ra.tail_cam   = ta.n_cam;
    ra.tail       = reinterpret_cast<const spd::TailArgs*>(tb);
    const int t_blocks = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)r.n_cu * t_per_cu, (n_tiles * (cp.chunks + 1) + 3) / 4));
    SP_HIP(hipEventRecord(r.ev0, c.stream));
    if (!cam_fold) SP_HIP(spd::chunk_camera(s->dev, a, r.n_cu, c.stream));
    SP_HIP(spd::launch_tail(s->dev, ra, 0, t_blocks, lds_bytes, c.stream));
    SP_HIP(spd::chunk_sum(s->dev, a, c.stream));
    c.launches = cam_fold ? 2 : 3;
    return SP_OK;
}

// Tail chunks (sp_mega.hpp, sp_device.hpp TailArgs): the K = tail_frac x n_tiles most expensive
// tiles of the order are rendered as sample chunks at the end of the queue.  DirectLighting at 3
// or 4 waves per SIMD with the tile order; the preps take the draw counts from the camera hits, or
// with an image light replay Light::sample on the stream (TailArgs replay); SP_TAIL_FRAC (0: off)
// and SP_TAIL_CHUNKS override.  Sets c.tail_k / c.tail_ch, m.a's tail fields and tail_sum's
// arguments; c.tail_k == 0: no tail chunks in this call.
static int plan_tail_chunks(RenderCall& c, MegaSetup& m, bool tail_replay, spd::ChunkArgs& tail_sum)
{
    sp_scene*      s = c.s;
    RenderScratch& r = s->scratch;
    const int64_t  n_tiles = c.tiles.n;
    const uint32_t spp_u   = c.p->samples_per_pixel;
    // automatic: one tile per persistent wave's worth (waves / n_tiles: 0.126 for the 1-GPU
    // 1080p frame, 0.25 for a 2-way shard, 0.38 for a 3-way one), within [SP_TAIL_FRAC, 0.4]
    // -- measured best 0.12-0.16, 0.2-0.3 and 0.4 there (profiles/r06/tail/); the environment's
    // SP_TAIL_FRAC instead (A/B runs); the caller's tail_fraction when set (< 0: off)
    float tail_frac = std::min(0.4f, std::max(SP_TAIL_FRAC, (float)((double)m.waves / (double)n_tiles)));
    if (c.hooks.tail_frac_set) tail_frac = c.hooks.tail_frac;
    if (c.p->tail_fraction != 0.0f) tail_frac = c.p->tail_fraction;
    c.tail_ch = c.hooks.tail_chunks;
    if (!(tail_frac > 0.0f)) return SP_OK;
    // ceil(frac x n), with frac the f32 caller value (0.05f x 5120 = 256.0000038: 256 tiles)
    const int64_t   k     = std::min<int64_t>(n_tiles, std::max<int64_t>(1, (int64_t)std::ceil((double)tail_frac * (double)n_tiles - 1e-3)));
    const ChunkPlan cp    = splan::chunk_plan(k, spp_u, std::max(1, c.tail_ch), s->dev.n_lights, c.image_light, c.hooks);
    const size_t    a_hdr = 256, a_rdy = ((size_t)k * 4 + 255) / 256 * 256;
    const size_t    need  = a_hdr + a_rdy + cp.b_hits + cp.b_L + cp.b_snap + cp.b_ctl;
    // the sample chunks' budget (chunk_max_gb, never more than the device can still give):
    // 20 GB for bunny's 4096 tail tiles (the store: 30 generations per pixel); a scene
    // with many lights (a store bound of 34 draws per light and sample) renders without
    // tail chunks rather than fail -- as it does when the allocation itself fails
    const double tail_budget = std::min(c.ck_max_gb * 1e9, (double)c.free_b + (double)r.tail_buf.cap);
    if ((double)need > tail_budget || r.tail_buf.reserve(need) != hipSuccess) return SP_OK;
    char*         base = r.tail_buf.as<char>();
    spd::TailArgs ta{};
    c.tail_k       = k;
    c.tail_ch      = (int)cp.chunks;
    ta.n_prep      = k;
    ta.replay      = tail_replay ? 1 : 0; // an image light: the preps replay Light::sample
    ta.n_items     = k * cp.chunks;
    ta.chunks      = (uint32_t)cp.chunks;
    ta.chunk_len   = cp.len;
    ta.gens_per_px = cp.gens;
    ta.n_px        = (size_t)k * 64;
    ta.ready       = reinterpret_cast<uint32_t*>(base + a_hdr);
    ta.hits        = reinterpret_cast<float4*>(base + a_hdr + a_rdy);
    ta.L           = reinterpret_cast<float*>(base + a_hdr + a_rdy + cp.b_hits);
    ta.gens        = reinterpret_cast<uint64_t*>(base + a_hdr + a_rdy + cp.b_hits + cp.b_L);
    ta.snap_ctl    = reinterpret_cast<uint32_t*>(base + a_hdr + a_rdy + cp.b_hits + cp.b_L + cp.b_snap);
    // the kernel reads TailArgs from device memory (stream-ordered behind the previous
    // call's kernels, which may still read it)
    SP_HIP(hipMemcpyAsync(base, &ta, sizeof(ta), hipMemcpyHostToDevice, c.stream));
    SP_HIP(hipMemsetAsync(ta.ready, 0, (size_t)k * 4, c.stream));
    m.a.tail_prep  = ta.n_prep;
    m.a.tail_items = ta.n_items;
    m.a.tail       = reinterpret_cast<const spd::TailArgs*>(base);
    tail_sum.tile_ids  = c.d_ids;
    tail_sum.num_tiles = k;
    tail_sum.tiles_x   = m.a.tiles_x;
    tail_sum.spp       = spp_u;
    tail_sum.n_px      = ta.n_px;
    tail_sum.L         = ta.L;
    tail_sum.out       = c.d_out;
    tail_sum.slot_map  = m.a.order; // chunk slot k is queue item k: tile slot order[k]
    return SP_OK;
}

static int run_megakernel(RenderCall& c)
{
    sp_scene*               s = c.s;
    RenderScratch&          r = s->scratch;
    const sp_render_params* p = c.p;
    const int64_t           n_tiles = c.tiles.n;
    MegaSetup m;
    if (int rc = mega_setup(s, spd::MegaFamily::Render, c.integ, p->waves_per_simd, c.d_ids, n_tiles, m)) return rc;
    SP_HIP(hipMemsetAsync(r.tile_counter.ptr, 0, sizeof(int32_t), c.stream));
    m.sc_run.merge_queries = (p->flags & SP_RENDER_PER_LANE_QUERIES) ? 0 : 1;
    m.a.out = c.d_out;
    m.a.spp = p->samples_per_pixel;
    SP_HIP(hipEventRecord(r.ev0, c.stream));
    // SP_TILE_DIAG=<file>: per-tile timeline {t0, t1, wave, item} (u64, s_memrealtime 100 MHz) and,
    // in a -DSP_MEGA_PROF build, shader clocks in trace / light sample / eval / occlusion
    DeviceScratch tdiag;
    if (c.hooks.tile_diag) {
        // the -DSP_WAVE_PROF / -DSP_TRAFFIC_DIAG builds add their totals into words 0..47
        const size_t words = std::max<size_t>((size_t)n_tiles * 8, 48);
        SP_HIP(tdiag.reserve(words * sizeof(unsigned long long)));
        SP_HIP(hipMemsetAsync(tdiag.ptr, 0, words * sizeof(unsigned long long), c.stream));
    }
    m.a.tile_diag = tdiag.as<unsigned long long>();
    // Tile order (order_tiles): the queue ordered by cost class (slower than `hoist` x the mean
    // first, the cheapest last), so the frame does not end with a few waves finishing expensive
    // tiles alone.  Used where it measured faster
    // (profiles/r03/ab_tile_order.txt, profiles/r04/tile_classes/): DirectLighting with many
    // tiles per persistent wave and a probe that costs little of the frame (bunny 1080p @ 256
    // spp, 7.9 tiles per wave; lucy; spheres 1024^2 @ 64 spp, 4 tiles per wave, loses 1 %);
    // IterativeRRNEE, whose tile costs spread wider (paths end at any depth), from 4 tiles per
    // wave and 16 spp (elf 1024^2 @ 16 spp +1.7 %; elf's 8-way shard +3 % with two classes, +5 % more with six).  DirectLighting and
    // IterativeRRNEE have probe kernels (sp_probe_*.hip); the other integrators render in queue
    // order.  sp_render_params.tile_order_factor > 0 forces it with that factor, < 0 turns it off.
    const bool    rrnee     = c.integ == SP_INTEGRATOR_ITERATIVE_RRNEE;
    const bool    tail_auto = c.plan.tail_auto;
    const int64_t waves     = (int64_t)m.waves;
    // (DirectLighting with tail chunks: from 3 tiles per wave, splan::tail_auto)
    float hoist = (n_tiles >= (rrnee ? 4 : 6) * waves && p->samples_per_pixel >= (rrnee ? 16u : 128u)) ? 2.0f : 0.0f;
    if (tail_auto && 2 * n_tiles >= 5 * waves) hoist = 2.0f; // the tail chunks need the order
    if (p->tile_order_factor != 0.0f) hoist = std::max(0.0f, p->tile_order_factor);
    if (hoist > 0.0f && n_tiles > waves && spd::has_probe(c.integ)) {
        SP_HIP(r.d_tile_time.reserve((size_t)n_tiles * sizeof(float))); // the pair grows together: one size
        SP_HIP(r.d_order.reserve((size_t)n_tiles * sizeof(int32_t)));
        // every 2nd slot timed where tail chunks follow and a wave takes 6 tiles or more (the others
        // interpolated by the order kernel: bunny +0.25 %, lucy +0.2 %); at 4 tiles per wave the
        // 2-way shard lost 2.5 % with it (spheres gained 0.6-0.8 %), and IterativeRRNEE, whose order
        // has no tail chunks behind it, lost 2-4 % on elf's shard (profiles/r06/tail/ab_probe_step*.log)
        int probe_step = (c.integ == SP_INTEGRATOR_DIRECT_LIGHTING && (tail_auto || p->tail_fraction > 0.0f) && n_tiles >= 6 * waves) ? 2 : 1;
        if (c.hooks.probe_step) probe_step = c.hooks.probe_step;
        // cost estimates blended with their queue neighbours only where those sit at known
        // image offsets: a whole frame, or a host list with a constant stride (the bench's list,
        // a rank's interleaved shard; order_neighbours); any other list keeps each tile's own time
        const int neighbours = splan::order_neighbours(p->tile_ids, c.tiles.listed, n_tiles, m.a.tiles_x);
        if (int rc = order_tiles(s, m, c.d_out, r.d_tile_time.as<float>(), r.d_order.as<int32_t>(), hoist, probe_step, neighbours, c.stream))
            return rc;
        m.a.order = r.d_order.as<int32_t>();
        c.launches += 2;
    }
    spd::ChunkArgs tail_sum{};
    // counts replayed on the stream (an image light, or SP_CHUNK_REPLAY): the 4-wave kernel only
    const bool tail_replay = !splan::chunk_plan(1, p->samples_per_pixel, 1, s->dev.n_lights, c.image_light, c.hooks).known_draws;
    if (c.integ == SP_INTEGRATOR_DIRECT_LIGHTING && (m.variant == 4 || (m.variant == 3 && !tail_replay)) && m.a.order)
        if (int rc = plan_tail_chunks(c, m, tail_replay, tail_sum)) return rc;
    if (c.timing) {
        if (!r.ev_render) SP_HIP(hipEventCreate(&r.ev_render[0]));
        SP_HIP(hipEventRecord(r.ev_render, c.stream));
    }
    if (c.tail_k > 0) {
        const int     t_var    = tail_replay ? -m.variant : m.variant; // -4: the replaying tail kernel
        const int     t_per_cu = spd::kernel_blocks_per_cu(spd::tail_kernel(t_var), m.lds_bytes);
        const int64_t t_need   = (n_tiles + m.a.tail_items + 3) / 4;
        const int     t_blocks = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)r.n_cu * t_per_cu, t_need));
        SP_HIP(spd::launch_tail(m.sc_run, m.a, t_var, t_blocks, m.lds_bytes, c.stream));
        SP_HIP(spd::chunk_sum(m.sc_run, tail_sum, c.stream));
        c.launches += 1;
    } else {
        SP_HIP(spd::launch_mega(m.family, m.sc_run, m.a, nullptr, nullptr, m.integ, m.variant, m.blocks, m.lds_bytes, c.stream));
    }
    if (tdiag.ptr) { // diagnostic: waits for the render
        SP_HIP(hipStreamSynchronize(c.stream));
        std::vector<unsigned long long> rec((size_t)n_tiles * 8);
        SP_HIP(hipMemcpy(rec.data(), tdiag.ptr, rec.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        if (FILE* f = std::fopen(c.hooks.tile_diag, "wb")) {
            std::fwrite(rec.data(), sizeof(unsigned long long), rec.size(), f);
            std::fclose(f);
        }
    }
    c.launches += 1;
    return SP_OK;
}

// The sample chunks count camera rays and samples on the host: one per inside pixel and sample
static int chunk_stats(const RenderCall& c, const unsigned long long (&ctr)[8], sp_render_stats* stats)
{
    const sp_scene*      s = c.s;
    std::vector<int32_t> ids;
    if (c.tiles.listed) {
        ids.resize((size_t)c.tiles.n);
        if (c.p->tile_ids) std::memcpy(ids.data(), c.p->tile_ids, ids.size() * sizeof(int32_t));
        else SP_HIP(hipMemcpy(ids.data(), c.p->d_tile_ids, ids.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    int64_t       inside = 0;
    const int32_t tw     = (s->dev.width + 7) / 8;
    for (int64_t sl = 0; sl < c.tiles.n; ++sl) {
        const int64_t t = c.tiles.listed ? ids[(size_t)sl] : sl;
        if (t < 0 || t >= c.tiles.total) continue;
        const int64_t x0 = (t % tw) * 8, y0 = (t / tw) * 8;
        inside += std::min<int64_t>(8, s->dev.width - x0) * std::min<int64_t>(8, s->dev.height - y0);
    }
    stats->samples = (unsigned long long)inside * c.p->samples_per_pixel;
    stats->rays    = (s->dev.max_depth > 0 ? stats->samples : 0ull) + ctr[1];
    return SP_OK;
}

static int render_tiles_impl(sp_scene* s, const sp_render_params* p, float* d_out, sp_render_stats* stats)
{
    if (int rc = validate_render(s, p, d_out)) return rc;
    SP_HIP(hipSetDevice(s->device));
    RenderScratch& r = s->scratch;
    RenderCall     c{ s, p, d_out, static_cast<hipStream_t>(p->stream), RenderHooks::from_env() };
    if (int rc = resolve_integrator(s, p->integrator, p->waves_per_simd, c.integ)) return rc;
    c.tiles = tile_list(s, p->tile_ids, p->d_tile_ids, p->num_tiles);
    if (int rc = check_tile_list(c.tiles, p->tile_ids)) return rc;
    c.d_ids  = p->d_tile_ids;
    c.timing = (p->flags & SP_RENDER_STAGE_TIMING) != 0;
    if (stats) *stats = sp_render_stats{};
    if (c.tiles.n == 0) return SP_OK;
    // the previous call on this scene may have used another stream: its work on the shared
    // scratch comes first (sp_scene::mu)
    if (r.done_rec) SP_HIP(hipStreamWaitEvent(c.stream, r.ev_done, 0));
    if (p->tile_ids)
        if (int rc = stage_tile_list(c)) return rc;
    if (int rc = device_cus(s)) return rc;
    if (int rc = plan_call(c)) return rc;
    SP_HIP(hipMemsetAsync(r.counters.ptr, 0, 8 * sizeof(unsigned long long), c.stream));
    const int pipeline = c.plan.pipeline;
    if (int rc = pipeline == SP_PIPELINE_WAVEFRONT       ? run_wavefront(c)
                 : pipeline == SP_PIPELINE_SAMPLE_CHUNKS ? run_chunks(c)
                                                         : run_megakernel(c))
        return rc;
    if (int rc = end_call(s, c.stream)) return rc;
    // stream order: without stats nothing waits -- the render is only enqueued
    if (!stats) return SP_OK;
    unsigned long long ctr[8];
    if (int rc = read_stats(s, pipeline, c.launches, stats, ctr)) return rc;
    if (pipeline == SP_PIPELINE_SAMPLE_CHUNKS)
        if (int rc = chunk_stats(c, ctr, stats)) return rc;
    stats->primary_hits = ctr[4];
    stats->parts        = c.parts_used;
    stats->tail_tiles   = (int32_t)c.tail_k;
    stats->tail_chunks  = c.tail_k > 0 ? c.tail_ch : 0;
    if (pipeline == SP_PIPELINE_MEGAKERNEL && c.timing) { // [0] the render kernel, [1] probe + tile order
        float render_ms = stats->kernel_ms;
        if (r.ev_render) SP_HIP(hipEventElapsedTime(&render_ms, r.ev_render, r.ev1));
        c.stage[0] = render_ms;
        c.stage[1] = stats->kernel_ms - render_ms;
    }
    for (int k = 0; k < 4; ++k) stats->stage_ms[k] = c.stage[k];
    return SP_OK;
}

int sp_render_tiles_host(sp_scene* s, const sp_render_params* p, float* h_out, sp_render_stats* stats)
{
    if (!s || !p || !h_out) return fail(SP_ERR_ARG, "null argument");
    if (s->device < 0) return fail(SP_ERR_STATE, "sp_scene_upload must be called before rendering");
    SP_HIP(hipSetDevice(s->device));
    const int64_t n = tile_list(s, p->tile_ids, p->d_tile_ids, p->num_tiles).n; // what the render writes
    return render_to_host(n, h_out, [&](float* d) { return sp_render_tiles(s, p, d, stats); });
}

// ---- many views in one launch (SP_HAS_VIEWS) -------------------------------------------------------

// Arguments, in the order their errors are promised; changes no state.  The tile count is the host
// scene's (the resident one's is equal), so the list rules hold before any upload.
static int validate_views(const sp_scene* s, const sp_view_params* p, const float* out, TileList& tiles)
{
    if (!s || !p || !out) return fail(SP_ERR_ARG, "null argument");
    if (p->struct_size != sizeof(sp_view_params)) return fail(SP_ERR_ARG, "sp_view_params.struct_size is not this library's");
    for (int32_t r : p->reserved)
        if (r != 0) return fail(SP_ERR_ARG, "sp_view_params.reserved must be 0");
    if ((p->flags & ~SP_RENDER_PER_LANE_QUERIES) != 0) return fail(SP_ERR_ARG, "unknown flags");
    if (p->num_views < 1) return fail(SP_ERR_ARG, "num_views < 1");
    if ((p->cameras != nullptr) == (p->d_cameras != nullptr)) return fail(SP_ERR_ARG, "give cameras (host) or d_cameras (device), one of them");
    if (reinterpret_cast<uintptr_t>(p->d_cameras) % 16 != 0) return fail(SP_ERR_ARG, "d_cameras must be 16-byte aligned");
    if (p->cameras)
        for (int32_t v = 0; v < p->num_views; ++v) {
            if (p->cameras[v].film_width != s->host->image_width || p->cameras[v].film_height != s->host->image_height)
                return fail(SP_ERR_ARG, "a view's film size is not the scene's image size");
            if (!camera_finite(p->cameras[v])) return fail(SP_ERR_ARG, "a view's transform is not finite");
        }
    if (p->tile_ids && p->d_tile_ids) return fail(SP_ERR_ARG, "give tile_ids (host) or d_tile_ids (device), not both");
    sp_tile_count(s->host->image_width, s->host->image_height, &tiles.total);
    tiles.listed = p->tile_ids || p->d_tile_ids;
    tiles.n      = tiles.listed ? p->num_tiles : tiles.total;
    if (int rc = check_tile_list(tiles, p->tile_ids)) return rc;
    if (p->samples_per_pixel == 0) return fail(SP_ERR_ARG, "samples_per_pixel must be > 0");
    if (s->device < 0) return fail(SP_ERR_STATE, "sp_scene_upload must be called before sp_render_views");
    return SP_OK;
}

// Host cameras to the device through a ring of pinned buffers of their own (stage_ids is the pattern)
static int stage_cameras(sp_scene* s, const sp_camera_desc* cams, int32_t n, hipStream_t stream, const spd::aff*& d_cams)
{
    RenderScratch& r     = s->scratch;
    const size_t   bytes = (size_t)n * sizeof(spd::aff);
    static_assert(sizeof(spd::aff) == 48 && sizeof(sp_affine) == 48, "twelve floats per camera");
    SP_HIP(r.d_cams.reserve(bytes));
    const int k = r.cams_next;
    r.cams_next = (k + 1) % RenderScratch::STAGE_RING;
    if (r.cams_rec[k]) SP_HIP(hipEventSynchronize(r.ev_cams[k]));
    SP_HIP(r.h_cams[k].reserve(bytes));
    for (int32_t v = 0; v < n; ++v) std::memcpy(r.h_cams[k].as<char>() + (size_t)v * 48, &cams[v].transform, 48);
    SP_HIP(hipMemcpyAsync(r.d_cams.ptr, r.h_cams[k].ptr, bytes, hipMemcpyHostToDevice, stream));
    SP_HIP(hipEventRecord(r.ev_cams[k], stream));
    r.cams_rec[k] = true;
    d_cams        = r.d_cams.as<spd::aff>();
    return SP_OK;
}

static int render_views_impl(sp_scene* s, const sp_view_params* p, float* d_out, sp_render_stats* stats)
{
    TileList tiles;
    if (int rc = validate_views(s, p, d_out, tiles)) return rc;
    int32_t integ = 0;
    if (int rc = resolve_integrator(s, p->integrator, p->waves_per_simd, integ)) return rc;
    if (integ == SP_INTEGRATOR_MANDELBROT) return fail(SP_ERR_UNSUPPORTED, "sp_render_views: Mandelbrot has no camera");
    if (tiles.n > 0 && (int64_t)p->num_views > (int64_t)INT32_MAX / tiles.n)
        return fail(SP_ERR_UNSUPPORTED, "sp_render_views: more than INT32_MAX queue items (num_views x num_tiles)");
    SP_HIP(hipSetDevice(s->device));
    RenderScratch&    r      = s->scratch;
    const hipStream_t stream = static_cast<hipStream_t>(p->stream);
    if (stats) *stats = sp_render_stats{};
    if (tiles.n == 0) return SP_OK;
    // the previous call on this scene may have used another stream (render_tiles_impl)
    if (r.done_rec) SP_HIP(hipStreamWaitEvent(stream, r.ev_done, 0));
    const int32_t* d_ids = p->d_tile_ids;
    if (p->tile_ids)
        if (int rc = stage_ids(s, p->tile_ids, tiles.n, stream, d_ids)) return rc;
    spd::ViewArgs vw{};
    vw.cameras        = reinterpret_cast<const spd::aff*>(p->d_cameras);
    vw.tiles_per_view = tiles.n;
    if (p->cameras)
        if (int rc = stage_cameras(s, p->cameras, p->num_views, stream, vw.cameras)) return rc;
    if (int rc = device_cus(s)) return rc;
    MegaSetup m;
    if (int rc = mega_setup(s, spd::MegaFamily::Views, integ, p->waves_per_simd, d_ids, (int64_t)p->num_views * tiles.n, m)) return rc;
    SP_HIP(hipMemsetAsync(r.counters.ptr, 0, 8 * sizeof(unsigned long long), stream));
    SP_HIP(hipMemsetAsync(r.tile_counter.ptr, 0, sizeof(int32_t), stream));
    m.sc_run.merge_queries = (p->flags & SP_RENDER_PER_LANE_QUERIES) ? 0 : 1;
    m.a.out = d_out;
    m.a.spp = p->samples_per_pixel;
    SP_HIP(hipEventRecord(r.ev0, stream));
    SP_HIP(spd::launch_mega(m.family, m.sc_run, m.a, nullptr, nullptr, m.integ, m.variant, m.blocks, m.lds_bytes, stream, &vw));
    if (int rc = end_call(s, stream)) return rc;
    if (!stats) return SP_OK; // stream order: only enqueued
    unsigned long long ctr[8];
    return read_stats(s, SP_PIPELINE_MEGAKERNEL, 1, stats, ctr);
}

int sp_render_views(sp_scene* s, const sp_view_params* p, float* d_out, sp_render_stats* stats)
{
    if (!s) return fail(SP_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lock(s->mu);
    try {
        return render_views_impl(s, p, d_out, stats);
    } catch (const std::exception& e) {
        return fail(SP_ERR_HIP, std::string("sp_render_views failed: ") + e.what());
    }
}

int sp_render_views_host(sp_scene* s, const sp_view_params* p, float* h_out, sp_render_stats* stats)
{
    TileList tiles;
    if (int rc = validate_views(s, p, h_out, tiles)) return rc; // (before any device buffer is made)
    if (tiles.n > 0 && (int64_t)p->num_views > (int64_t)INT32_MAX / tiles.n)
        return fail(SP_ERR_UNSUPPORTED, "sp_render_views: more than INT32_MAX queue items (num_views x num_tiles)");
    SP_HIP(hipSetDevice(s->device));
    return render_to_host((int64_t)p->num_views * tiles.n, h_out, [&](float* d) { return sp_render_views(s, p, d, stats); });
}

// ---- radiance queries (SP_HAS_RADIANCE_QUERY; sp_radiance.hpp) --------------------------------------

// Arguments, in the order their errors are promised; changes no state.  rays: the device buffer, or
// the host form's array (device_pointers false: no alignment is asked of it).  The waves_per_simd
// range is the integrator's, which the host scene names without an upload; an integrator that does
// not resolve is refused where sp_render_tiles refuses it, after the residency.
static int validate_radiance(const sp_scene* s, const sp_radiance_query* q, const sp_radiance_ray* rays, const float* out,
                             bool device_pointers)
{
    if (!s || !q || !out) return fail(SP_ERR_ARG, "null argument");
    if (q->struct_size != sizeof(sp_radiance_query)) return fail(SP_ERR_ARG, "sp_radiance_query.struct_size is not this library's");
    if (q->reserved0 != 0) return fail(SP_ERR_ARG, "sp_radiance_query.reserved must be 0");
    for (int32_t r : q->reserved)
        if (r != 0) return fail(SP_ERR_ARG, "sp_radiance_query.reserved must be 0");
    if ((q->flags & ~SP_RENDER_PER_LANE_QUERIES) != 0) return fail(SP_ERR_ARG, "unknown flags");
    if (q->num_rays < 0) return fail(SP_ERR_ARG, "num_rays < 0");
    if (q->num_rays > 0 && !rays) return fail(SP_ERR_ARG, device_pointers ? "d_rays is NULL" : "h_rays is NULL");
    if (device_pointers && reinterpret_cast<uintptr_t>(rays) % 16 != 0) return fail(SP_ERR_ARG, "d_rays must be 16-byte aligned");
    if (q->samples_per_ray == 0) return fail(SP_ERR_ARG, "samples_per_ray must be > 0");
    int32_t integ = q->integrator != SP_INTEGRATOR_NOT_SPECIFIED ? q->integrator : s->host->integrator;
    if (integ == SP_INTEGRATOR_NOT_SPECIFIED) integ = SP_INTEGRATOR_DIRECT_LIGHTING;
    if (q->waves_per_simd != 0 && integ >= SP_INTEGRATOR_MANDELBROT && integ <= SP_INTEGRATOR_WHITTED) {
        int32_t same = 0;
        if (int rc = resolve_integrator(s, integ, q->waves_per_simd, same)) return rc;
    }
    if (s->device < 0) return fail(SP_ERR_STATE, "sp_scene_upload must be called before sp_scene_radiance_rays");
    return SP_OK;
}

// after validate_radiance, with the scene's lock held
static int radiance_rays_impl(sp_scene* s, const sp_radiance_query* q, float* d_out, sp_render_stats* stats)
{
    int32_t integ = 0;
    if (int rc = resolve_integrator(s, q->integrator, q->waves_per_simd, integ)) return rc;
    if (integ == SP_INTEGRATOR_MANDELBROT) return fail(SP_ERR_UNSUPPORTED, "sp_scene_radiance_rays: Mandelbrot has no ray");
    const int64_t items = q->num_rays / 64 + (q->num_rays % 64 != 0);
    if (items > (int64_t)INT32_MAX)
        return fail(SP_ERR_UNSUPPORTED, "sp_scene_radiance_rays: more than INT32_MAX queue items of 64 rays");
    SP_HIP(hipSetDevice(s->device));
    RenderScratch&    r      = s->scratch;
    const hipStream_t stream = static_cast<hipStream_t>(q->stream);
    if (stats) *stats = sp_render_stats{};
    if (q->num_rays == 0) return SP_OK;
    // the previous call on this scene may have used another stream (render_tiles_impl)
    if (r.done_rec) SP_HIP(hipStreamWaitEvent(stream, r.ev_done, 0));
    if (int rc = device_cus(s)) return rc;
    MegaSetup m;
    if (int rc = mega_setup(s, spd::MegaFamily::Radiance, integ, q->waves_per_simd, nullptr, items, m)) return rc;
    SP_HIP(hipMemsetAsync(r.counters.ptr, 0, 8 * sizeof(unsigned long long), stream));
    SP_HIP(hipMemsetAsync(r.tile_counter.ptr, 0, sizeof(int32_t), stream));
    m.sc_run.merge_queries = (q->flags & SP_RENDER_PER_LANE_QUERIES) ? 0 : 1;
    m.a.out = d_out;
    m.a.spp = q->samples_per_ray;
    spd::RadianceArgs ra{};
    ra.rays     = q->d_rays;
    ra.num_rays = q->num_rays;
    SP_HIP(hipEventRecord(r.ev0, stream));
    SP_HIP(spd::launch_radiance(m.sc_run, m.a, ra, m.integ, m.variant, m.blocks, m.lds_bytes, stream));
    if (int rc = end_call(s, stream)) return rc;
    if (!stats) return SP_OK; // stream order: only enqueued
    unsigned long long ctr[8];
    return read_stats(s, SP_PIPELINE_MEGAKERNEL, 1, stats, ctr);
}

int sp_scene_radiance_rays(sp_scene* s, const sp_radiance_query* q, float* d_out, sp_render_stats* stats)
{
    if (!s) return fail(SP_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lock(s->mu);
    try {
        if (int rc = validate_radiance(s, q, q ? q->d_rays : nullptr, d_out, true)) return rc;
        return radiance_rays_impl(s, q, d_out, stats);
    } catch (const std::exception& e) {
        return fail(SP_ERR_HIP, std::string("sp_scene_radiance_rays failed: ") + e.what());
    }
}

// the host form with the scene's lock held: the same refusals in the same order on the host arrays
// as given, then device buffers of its own around the device form (trace_rays_host_impl's pattern)
static int radiance_rays_host_impl(sp_scene* s, const sp_radiance_query* q, const sp_radiance_ray* h_rays, float* h_out,
                                   sp_render_stats* stats)
{
    if (int rc = validate_radiance(s, q, h_rays, h_out, false)) return rc;
    sp_radiance_query dq = *q;
    dq.d_rays = nullptr;
    dq.stream = nullptr; // with the blocking copies below, as render_to_host
    const size_t  n = (size_t)q->num_rays;
    DeviceScratch d_rays, d_out;
    if (n) {
        SP_HIP(hipSetDevice(s->device));
        SP_HIP(d_rays.reserve(n * sizeof(sp_radiance_ray)));
        SP_HIP(d_out.reserve(n * 3 * sizeof(float)));
        SP_HIP(hipMemcpy(d_rays.ptr, h_rays, n * sizeof(sp_radiance_ray), hipMemcpyHostToDevice));
        dq.d_rays = d_rays.as<sp_radiance_ray>();
    }
    if (int rc = radiance_rays_impl(s, &dq, d_out.as<float>(), stats)) return rc;
    if (n) SP_HIP(hipMemcpy(h_out, d_out.ptr, n * 3 * sizeof(float), hipMemcpyDeviceToHost));
    return SP_OK;
}

int sp_scene_radiance_rays_host(sp_scene* s, const sp_radiance_query* q, const sp_radiance_ray* h_rays, float* h_out,
                                sp_render_stats* stats)
{
    if (!s) return fail(SP_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lock(s->mu); // residency is decided, and kept, under the scene's lock
    try {
        return radiance_rays_host_impl(s, q, h_rays, h_out, stats);
    } catch (const std::exception& e) {
        return fail(SP_ERR_HIP, std::string("sp_scene_radiance_rays_host failed: ") + e.what());
    }
}

// ---- progressive renders (sp_progress) ---------------------------------------------------------

// pixel (x, y) of record slot * 64 + m; false: outside the image (a clipped border tile, or a
// device list's id outside the frame)
static bool progress_pixel(const sp_progress* g, int64_t slot, uint32_t m, int32_t& x, int32_t& y)
{
    const int32_t tw    = (g->width + 7) / 8;
    const int64_t total = (int64_t)tw * ((g->height + 7) / 8);
    const int64_t t     = g->listed ? g->h_ids[(size_t)slot] : slot;
    if (t < 0 || t >= total) return false;
    uint32_t a = m & 0x55u, b = (m >> 1) & 0x55u;
    a = (a | (a >> 1)) & 0x33u; a = (a | (a >> 2)) & 0x0fu;
    b = (b | (b >> 1)) & 0x33u; b = (b | (b >> 2)) & 0x0fu;
    x = (int32_t)(t % tw) * 8 + (int32_t)a;
    y = (int32_t)(t / tw) * 8 + (int32_t)b;
    return x < g->width && y < g->height;
}

static int progress_live(const sp_progress* g)
{
    const sp_scene* s = g->scene;
    if (s->generation != g->generation || s->device != g->device)
        return fail(SP_ERR_STATE, "the scene was uploaded again or resized after sp_progress_create");
    return SP_OK;
}

static int progress_create_impl(sp_scene* s, const sp_progress_params* p, sp_progress** out, bool adaptive = false)
{
    if (p->struct_size != sizeof(sp_progress_params)) return fail(SP_ERR_ARG, "sp_progress_params.struct_size is not this library's");
    if (p->reserved[0] != 0 || p->reserved[1] != 0) return fail(SP_ERR_ARG, "sp_progress_params.reserved must be 0");
    if (p->tile_ids && p->d_tile_ids) return fail(SP_ERR_ARG, "give tile_ids (host) or d_tile_ids (device), not both");
    if (p->tile_order_factor != p->tile_order_factor) return fail(SP_ERR_ARG, "tile_order_factor is NaN");
    if (s->device < 0) return fail(SP_ERR_STATE, "sp_scene_upload must be called before sp_progress_create");
    int32_t integ = 0;
    if (int rc = resolve_integrator(s, p->integrator, p->waves_per_simd, integ)) return rc;
    const TileList tiles = tile_list(s, p->tile_ids, p->d_tile_ids, p->num_tiles);
    if (int rc = check_tile_list(tiles, p->tile_ids)) return rc;
    const bool    listed  = tiles.listed;
    const int64_t n_tiles = tiles.n;
    SP_HIP(hipSetDevice(s->device));
    std::unique_ptr<sp_progress> g(new sp_progress());
    g->scene        = s;
    g->generation   = s->generation;
    g->device       = s->device;
    g->integ        = integ;
    g->waves_req    = p->waves_per_simd;
    g->order_factor = p->tile_order_factor;
    g->listed       = listed;
    g->n_tiles      = n_tiles;
    g->width        = s->dev.width;
    g->height       = s->dev.height;
    const size_t nt = (size_t)std::max<int64_t>(1, n_tiles);
    if (listed) {
        g->h_ids.assign(nt, 0);
        if (p->tile_ids) std::memcpy(g->h_ids.data(), p->tile_ids, (size_t)n_tiles * sizeof(int32_t));
        else if (n_tiles > 0)
            SP_HIP(hipMemcpy(g->h_ids.data(), p->d_tile_ids, (size_t)n_tiles * sizeof(int32_t), hipMemcpyDeviceToHost));
        SP_HIP(g->alloc(&g->d_ids, nt * sizeof(int32_t), false));
        SP_HIP(hipMemcpy(g->d_ids, g->h_ids.data(), nt * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    // zeroed: pixels outside the image stay zero and export as zero records
    SP_HIP(g->alloc(&g->st.gen, nt * (size_t)spd::MT_GEN_WORDS * 8));
    SP_HIP(g->alloc(&g->st.pos, nt * 64 * 4));
    SP_HIP(g->alloc(&g->st.draws, nt * 64 * 8));
    SP_HIP(g->alloc(&g->st.sum, nt * 192 * 4));
    if (adaptive) {
        g->adaptive = true;
        const size_t b_px = nt * 64 * 4, b_tile = nt * 4;
        SP_HIP(g->alloc(&g->ad.mean, b_px)); // as the sums: zero outside the image
        SP_HIP(g->alloc(&g->ad.m2, b_px));
        SP_HIP(g->alloc(&g->ad.done, b_tile));
        SP_HIP(g->alloc(&g->ad.err, b_tile));
        SP_HIP(g->alloc(&g->ad.flag, b_tile));
        SP_HIP(g->alloc(&g->ad.active, b_tile));
        SP_HIP(g->alloc(&g->ad.n_active, sizeof(int32_t)));
        g->h_inside.assign(nt, 0);
        int32_t x, y;
        for (int64_t sl = 0; sl < n_tiles; ++sl)
            for (uint32_t m = 0; m < 64; ++m) g->h_inside[(size_t)sl] += progress_pixel(g.get(), sl, m, x, y) ? 1 : 0;
    }
    *out = g.release();
    return SP_OK;
}

int sp_progress_create(sp_scene* s, const sp_progress_params* p, sp_progress** out)
{
    if (!s || !p || !out) return fail(SP_ERR_ARG, "null argument");
    *out = nullptr;
    std::lock_guard<std::mutex> lock(s->mu);
    try {
        return progress_create_impl(s, p, out);
    } catch (const std::exception& e) {
        return fail(SP_ERR_HIP, std::string("sp_progress_create failed: ") + e.what());
    }
}

int sp_progress_create_adaptive(sp_scene* s, const sp_progress_params* p, sp_progress** out)
{
    if (!s || !p || !out) return fail(SP_ERR_ARG, "null argument");
    *out = nullptr;
    std::lock_guard<std::mutex> lock(s->mu);
    try {
        return progress_create_impl(s, p, out, true);
    } catch (const std::exception& e) {
        return fail(SP_ERR_HIP, std::string("sp_progress_create_adaptive failed: ") + e.what());
    }
}

void sp_progress_free(sp_progress* g) { delete g; }

// After the object's queued work: the tile counts, and optionally the errors of the last selection.
static int adaptive_fetch(sp_progress* g, std::vector<uint32_t>& done, std::vector<float>* err)
{
    sp_scene* s = g->scene;
    SP_HIP(hipSetDevice(s->device));
    if (int rc = wait_done(s)) return rc;
    done.assign((size_t)g->n_tiles, 0u);
    if (g->n_tiles == 0) return SP_OK;
    SP_HIP(hipMemcpy(done.data(), g->ad.done, done.size() * 4, hipMemcpyDeviceToHost));
    if (err) {
        err->assign((size_t)g->n_tiles, 0.0f);
        SP_HIP(hipMemcpy(err->data(), g->ad.err, err->size() * 4, hipMemcpyDeviceToHost));
    }
    return SP_OK;
}

// A round's rule on an adaptive object (sp_adaptive_round); a uniform pass (sp_progress_render) is
// the rule that selects every tile: min = max = UINT32_MAX, step = more_samples.
struct AdaptRound {
    float               threshold, floor;
    uint32_t            min_samples, max_samples, step;
    bool                uniform;
    sp_adaptive_result* result;
};

// rd: nullptr on a plain object
static int progress_render_impl(sp_progress* g, uint32_t more, hipStream_t stream, float* d_out, sp_render_stats* stats,
                                const AdaptRound* rd = nullptr)
{
    sp_scene*      s = g->scene;
    RenderScratch& r = s->scratch;
    if (int rc = progress_live(g)) return rc;
    if (more == 0) return fail(SP_ERR_ARG, "more_samples must be > 0");
    if ((!rd || rd->uniform) && (uint64_t)g->st.n0 + more > UINT32_MAX)
        return fail(SP_ERR_ARG, "more than UINT32_MAX samples in all");
    if (stats) *stats = sp_render_stats{};
    if (rd && rd->result) *rd->result = sp_adaptive_result{};
    SP_HIP(hipSetDevice(s->device));
    const int64_t n_tiles = g->n_tiles;
    // an adaptive object's count bound after this call (st.n0: no tile has more)
    const uint32_t n0_after = !rd || rd->uniform ? g->st.n0 + more
                                                 : std::max(g->st.n0, (uint32_t)std::min<uint64_t>((uint64_t)g->st.n0 + more, rd->max_samples));
    if (n_tiles == 0) {
        g->st.n0 = n0_after;
        return SP_OK;
    }
    // the scene's scratch (mt_state, counters) is shared with sp_render_tiles: same ordering
    if (r.done_rec) SP_HIP(hipStreamWaitEvent(stream, r.ev_done, 0));
    if (int rc = device_cus(s)) return rc;
    MegaSetup m;
    if (int rc = mega_setup(s, rd ? spd::MegaFamily::Adapt : spd::MegaFamily::Resume, g->integ, g->waves_req, g->d_ids, n_tiles, m))
        return rc;
    SP_HIP(hipMemsetAsync(r.counters.ptr, 0, 8 * sizeof(unsigned long long), stream));
    SP_HIP(hipMemsetAsync(r.tile_counter.ptr, 0, sizeof(int32_t), stream));
    m.sc_run.merge_queries = 1;
    m.a.out = d_out;
    m.a.spp = more; // (an adaptive call: at most; a tile's own count decides, AdaptArgs)
    SP_HIP(hipEventRecord(r.ev0, stream));
    int launches = 1;
    // Tile order (run_megakernel): the one-sample probe runs in the first call and its order is
    // kept -- it only permutes the tiles.  Automatic from the same tiles per wave as a one-shot
    // render (whose samples threshold has no counterpart here: a call does not know the total).
    if (!g->order_tried) {
        g->order_tried = true;
        const bool rrnee = g->integ == SP_INTEGRATOR_ITERATIVE_RRNEE;
        float      hoist = n_tiles >= (rrnee ? 4 : 6) * (int64_t)m.waves ? 2.0f : 0.0f;
        if (g->order_factor != 0.0f) hoist = std::max(0.0f, g->order_factor);
        if (hoist > 0.0f && n_tiles > (int64_t)m.waves && spd::has_probe(g->integ)) {
            SP_HIP(g->alloc(&g->d_tile_time, (size_t)n_tiles * sizeof(float), false));
            SP_HIP(g->alloc(&g->d_order, (size_t)n_tiles * sizeof(int32_t), false));
            const int neighbours = splan::order_neighbours(g->listed ? g->h_ids.data() : nullptr, g->listed, n_tiles, m.a.tiles_x);
            if (int rc = order_tiles(s, m, nullptr, g->d_tile_time, g->d_order, hoist, 1, neighbours, stream)) return rc;
            g->ordered = true;
            launches += 2;
        }
    }
    m.a.order = g->ordered ? g->d_order : nullptr;
    spd::AdaptArgs ad = g->ad;
    if (rd) {
        // errors and the selection, the selected slots in the kept tile order, the render kernel on
        // that list (its length stays on the device), then the image of the tiles it left alone
        spd::SelectArgs sa{};
        sa.tile_ids    = g->d_ids;
        sa.num_tiles   = n_tiles;
        sa.tiles_x     = m.a.tiles_x;
        sa.width       = s->dev.width;
        sa.height      = s->dev.height;
        sa.threshold   = rd->threshold;
        sa.floor       = rd->floor;
        sa.min_samples = rd->min_samples;
        sa.max_samples = rd->max_samples;
        ad.step        = rd->step;
        ad.cap         = rd->max_samples;
        SP_HIP(spd::launch_adapt_select(ad, sa, ad.err, ad.flag, stream));
        SP_HIP(spd::launch_adapt_compact(ad, m.a.order, n_tiles, stream));
        launches += 2;
    }
    SP_HIP(spd::launch_mega(m.family, m.sc_run, m.a, &g->st, &ad, m.integ, m.variant, m.blocks, m.lds_bytes, stream));
    if (rd && d_out && !rd->uniform) {
        SP_HIP(spd::launch_adapt_resolve(g->st, ad, true, n_tiles, d_out, stream));
        launches += 1;
    }
    if (int rc = end_call(s, stream)) return rc;
    g->st.n0 = n0_after;
    if (rd && rd->result) {
        sp_adaptive_result&   res = *rd->result;
        std::vector<uint32_t> done;
        std::vector<float>    err;
        if (int rc = adaptive_fetch(g, done, &err)) return rc;
        int32_t n_act = 0;
        SP_HIP(hipMemcpy(&n_act, g->ad.n_active, sizeof(n_act), hipMemcpyDeviceToHost));
        res.active_tiles = n_act;
        res.min_done     = UINT32_MAX;
        for (int64_t i = 0; i < n_tiles; ++i) {
            res.samples_total += (uint64_t)done[(size_t)i] * g->h_inside[(size_t)i];
            res.min_done  = std::min(res.min_done, done[(size_t)i]);
            res.max_done  = std::max(res.max_done, done[(size_t)i]);
            res.max_error = std::max(res.max_error, err[(size_t)i]);
        }
        g->st.n0 = res.max_done;
    }
    if (stats) {
        unsigned long long ctr[8];
        if (int rc = read_stats(s, SP_PIPELINE_MEGAKERNEL, launches, stats, ctr)) return rc;
    }
    return SP_OK;
}

int sp_progress_render(sp_progress* g, uint32_t more_samples, void* stream, float* d_out, sp_render_stats* stats)
{
    if (!g) return fail(SP_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lock(g->scene->mu);
    try {
        if (g->adaptive) { // every tile gets more_samples from its own count
            const AdaptRound all{ 0.0f, 0.01f, UINT32_MAX, UINT32_MAX, more_samples, true, nullptr };
            return progress_render_impl(g, more_samples, static_cast<hipStream_t>(stream), d_out, stats, &all);
        }
        return progress_render_impl(g, more_samples, static_cast<hipStream_t>(stream), d_out, stats);
    } catch (const std::exception& e) {
        return fail(SP_ERR_HIP, std::string("sp_progress_render failed: ") + e.what());
    }
}

int sp_progress_render_host(sp_progress* g, uint32_t more_samples, float* h_out, sp_render_stats* stats)
{
    if (!g || !h_out) return fail(SP_ERR_ARG, "null argument");
    if (g->scene->device < 0) return fail(SP_ERR_STATE, "the scene is no longer uploaded");
    SP_HIP(hipSetDevice(g->scene->device));
    return render_to_host(g->n_tiles, h_out, [&](float* d) { return sp_progress_render(g, more_samples, nullptr, d, stats); });
}

int sp_progress_samples(const sp_progress* g, uint32_t* out)
{
    if (!g || !out) return fail(SP_ERR_ARG, "null argument");
    *out = g->st.n0;
    if (g->adaptive) { // the largest tile count (waits for the object's queued work)
        std::lock_guard<std::mutex> lock(g->scene->mu);
        std::vector<uint32_t>       done;
        if (int rc = progress_live(g)) return rc;
        if (int rc = adaptive_fetch(const_cast<sp_progress*>(g), done, nullptr)) return rc;
        *out = 0;
        for (uint32_t c : done) *out = std::max(*out, c);
        if (g->n_tiles == 0) *out = g->st.n0;
    }
    return SP_OK;
}

int sp_progress_device_bytes(const sp_progress* g, int64_t* out)
{
    if (!g || !out) return fail(SP_ERR_ARG, "null argument");
    *out = g->bytes;
    return SP_OK;
}

// Export / import move PROGRESS_BATCH tiles' generations at a time through a host buffer in the
// device layout (160 KB per tile) and permute them on the host.
static constexpr int64_t PROGRESS_BATCH = 128;

static int progress_export_impl(sp_progress* g, sp_pixel_state* h, int64_t capacity, uint32_t* samples)
{
    sp_scene* s = g->scene;
    if (int rc = progress_live(g)) return rc;
    const int64_t n_px = g->n_tiles * 64;
    if (capacity < n_px) return fail(SP_ERR_ARG, "capacity below num_tiles * 64 records");
    *samples = g->st.n0;
    if (n_px == 0) return SP_OK;
    SP_HIP(hipSetDevice(s->device));
    if (int rc = wait_done(s)) return rc;
    std::vector<uint32_t> tile_done; // an adaptive object: each tile has its own count
    if (g->adaptive) {
        if (int rc = adaptive_fetch(g, tile_done, nullptr)) return rc;
        *samples = *std::max_element(tile_done.begin(), tile_done.end());
    }
    const uint32_t any_done = *samples;
    std::vector<uint32_t>           pos((size_t)n_px);
    std::vector<unsigned long long> draws((size_t)n_px);
    std::vector<float>              sum((size_t)g->n_tiles * 192);
    SP_HIP(hipMemcpy(pos.data(), g->st.pos, pos.size() * 4, hipMemcpyDeviceToHost));
    SP_HIP(hipMemcpy(draws.data(), g->st.draws, draws.size() * 8, hipMemcpyDeviceToHost));
    SP_HIP(hipMemcpy(sum.data(), g->st.sum, sum.size() * 4, hipMemcpyDeviceToHost));
    std::vector<uint64_t> gen((size_t)std::min(PROGRESS_BATCH, g->n_tiles) * spd::MT_GEN_WORDS);
    for (int64_t t0 = 0; t0 < g->n_tiles; t0 += PROGRESS_BATCH) {
        const int64_t nb = std::min(PROGRESS_BATCH, g->n_tiles - t0);
        if (any_done > 0)
            SP_HIP(hipMemcpy(gen.data(), g->st.gen + (size_t)t0 * spd::MT_GEN_WORDS, (size_t)nb * spd::MT_GEN_WORDS * 8,
                             hipMemcpyDeviceToHost));
        for (int64_t sl = t0; sl < t0 + nb; ++sl)
            for (uint32_t m = 0; m < 64; ++m) {
                sp_pixel_state& r = h[sl * 64 + m];
                std::memset(&r, 0, sizeof(r));
                int32_t x, y;
                if (!progress_pixel(g, sl, m, x, y)) continue;
                if ((g->adaptive ? tile_done[(size_t)sl] : g->st.n0) == 0) { // nothing rendered yet: the seeded engine (main.cpp:73), _M_p = n
                    spm::Mt64 e;
                    spm::mt_init(e, (((uint32_t)x << 16u) | (uint32_t)y) ^ 0xb0ae9d99u);
                    std::memcpy(r.mt, e.x, sizeof(r.mt));
                    r.mt_pos = spm::MT_N;
                    continue;
                }
                const uint64_t* b = gen.data() + (size_t)(sl - t0) * spd::MT_GEN_WORDS + (size_t)m * spd::MT_BLK;
                for (int k = 0; k < spm::MT_N; ++k) r.mt[k] = b[spd::mt_off(k)];
                r.mt_pos = pos[(size_t)sl * 64 + m];
                r.draws  = draws[(size_t)sl * 64 + m];
                for (int c = 0; c < 3; ++c) r.sum[c] = sum[(size_t)sl * 192 + (size_t)c * 64 + m];
            }
    }
    return SP_OK;
}

int sp_progress_export(sp_progress* g, sp_pixel_state* h_states, int64_t capacity, uint32_t* samples)
{
    if (!g || !h_states || !samples) return fail(SP_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lock(g->scene->mu);
    try {
        return progress_export_impl(g, h_states, capacity, samples);
    } catch (const std::exception& e) {
        return fail(SP_ERR_HIP, std::string("sp_progress_export failed: ") + e.what());
    }
}

static int progress_import_impl(sp_progress* g, const sp_pixel_state* h, int64_t count, uint32_t samples)
{
    sp_scene* s = g->scene;
    if (int rc = progress_live(g)) return rc;
    const int64_t n_px = g->n_tiles * 64;
    if (count != n_px) return fail(SP_ERR_ARG, "count is not num_tiles * 64 records");
    int32_t x, y;
    for (int64_t i = 0; i < n_px; ++i) { // everything is checked before anything is written
        if (!progress_pixel(g, i / 64, (uint32_t)(i % 64), x, y)) continue;
        if (h[i].mt_pos > (uint64_t)spm::MT_N) return fail(SP_ERR_ARG, "sp_pixel_state.mt_pos above 312");
        if (h[i].reserved != 0) return fail(SP_ERR_ARG, "sp_pixel_state.reserved must be 0");
    }
    if (n_px == 0) {
        g->st.n0 = samples;
        return SP_OK;
    }
    SP_HIP(hipSetDevice(s->device));
    if (int rc = wait_done(s)) return rc;
    if (g->adaptive) { // every tile at `samples`, no statistics: sp_adaptive_import brings both
        const std::vector<uint32_t> all((size_t)g->n_tiles, samples);
        SP_HIP(hipMemcpy(g->ad.done, all.data(), all.size() * 4, hipMemcpyHostToDevice));
        SP_HIP(hipMemset(g->ad.mean, 0, (size_t)n_px * 4));
        SP_HIP(hipMemset(g->ad.m2, 0, (size_t)n_px * 4));
    }
    std::vector<uint32_t>           pos((size_t)n_px, 0u);
    std::vector<unsigned long long> draws((size_t)n_px, 0ull);
    std::vector<float>              sum((size_t)g->n_tiles * 192, 0.0f);
    std::vector<uint64_t>           gen((size_t)std::min(PROGRESS_BATCH, g->n_tiles) * spd::MT_GEN_WORDS);
    for (int64_t t0 = 0; t0 < g->n_tiles; t0 += PROGRESS_BATCH) {
        const int64_t nb = std::min(PROGRESS_BATCH, g->n_tiles - t0);
        std::fill(gen.begin(), gen.end(), 0ull);
        for (int64_t sl = t0; sl < t0 + nb; ++sl)
            for (uint32_t m = 0; m < 64; ++m) {
                if (samples == 0 || !progress_pixel(g, sl, m, x, y)) continue; // (0 samples: the first call seeds)
                const sp_pixel_state& r = h[sl * 64 + m];
                uint64_t*             b = gen.data() + (size_t)(sl - t0) * spd::MT_GEN_WORDS + (size_t)m * spd::MT_BLK;
                for (int k = 0; k < spm::MT_N; ++k) b[spd::mt_off(k)] = r.mt[k];
                pos[(size_t)sl * 64 + m]   = (uint32_t)r.mt_pos;
                draws[(size_t)sl * 64 + m] = r.draws;
                for (int c = 0; c < 3; ++c) sum[(size_t)sl * 192 + (size_t)c * 64 + m] = r.sum[c];
            }
        SP_HIP(hipMemcpy(g->st.gen + (size_t)t0 * spd::MT_GEN_WORDS, gen.data(), (size_t)nb * spd::MT_GEN_WORDS * 8,
                         hipMemcpyHostToDevice));
    }
    SP_HIP(hipMemcpy(g->st.pos, pos.data(), pos.size() * 4, hipMemcpyHostToDevice));
    SP_HIP(hipMemcpy(g->st.draws, draws.data(), draws.size() * 8, hipMemcpyHostToDevice));
    SP_HIP(hipMemcpy(g->st.sum, sum.data(), sum.size() * 4, hipMemcpyHostToDevice));
    g->st.n0 = samples;
    return SP_OK;
}

int sp_progress_import(sp_progress* g, const sp_pixel_state* h_states, int64_t count, uint32_t samples)
{
    if (!g || !h_states) return fail(SP_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lock(g->scene->mu);
    try {
        return progress_import_impl(g, h_states, count, samples);
    } catch (const std::exception& e) {
        return fail(SP_ERR_HIP, std::string("sp_progress_import failed: ") + e.what());
    }
}

// ---- adaptive sampling (adaptive progress objects) ---------------------------------------------

static int adaptive_object(const sp_progress* g)
{
    if (!g->adaptive) return fail(SP_ERR_STATE, "not an adaptive progress object (sp_progress_create_adaptive)");
    return progress_live(g);
}

static int adaptive_round_params(const sp_adaptive_params* p, sp_adaptive_result* result, AdaptRound& rd)
{
    if (p->struct_size != sizeof(sp_adaptive_params)) return fail(SP_ERR_ARG, "sp_adaptive_params.struct_size is not this library's");
    if (p->reserved[0] != 0 || p->reserved[1] != 0) return fail(SP_ERR_ARG, "sp_adaptive_params.reserved must be 0");
    if (!(p->threshold >= 0.0f) || !std::isfinite(p->threshold)) return fail(SP_ERR_ARG, "threshold must be finite and >= 0");
    if (!(p->floor >= 0.0f) || !std::isfinite(p->floor)) return fail(SP_ERR_ARG, "floor must be finite and >= 0");
    if (p->step < 1) return fail(SP_ERR_ARG, "step must be >= 1");
    if (p->max_samples < 1 || p->min_samples > p->max_samples) return fail(SP_ERR_ARG, "need 1 <= max_samples and min_samples <= max_samples");
    rd = AdaptRound{ p->threshold, p->floor == 0.0f ? 0.01f : p->floor, p->min_samples, p->max_samples, p->step, false, result };
    return SP_OK;
}

int sp_adaptive_round(sp_progress* g, const sp_adaptive_params* p, void* stream, float* d_out, sp_render_stats* stats,
                      sp_adaptive_result* result)
{
    if (!g || !p) return fail(SP_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lock(g->scene->mu);
    try {
        if (int rc = adaptive_object(g)) return rc;
        AdaptRound rd{};
        if (int rc = adaptive_round_params(p, result, rd)) return rc;
        return progress_render_impl(g, rd.step, static_cast<hipStream_t>(stream), d_out, stats, &rd);
    } catch (const std::exception& e) {
        return fail(SP_ERR_HIP, std::string("sp_adaptive_round failed: ") + e.what());
    }
}

int sp_adaptive_round_host(sp_progress* g, const sp_adaptive_params* p, float* h_out, sp_render_stats* stats,
                           sp_adaptive_result* result)
{
    if (!g || !p || !h_out) return fail(SP_ERR_ARG, "null argument");
    if (g->scene->device < 0) return fail(SP_ERR_STATE, "the scene is no longer uploaded");
    SP_HIP(hipSetDevice(g->scene->device));
    return render_to_host(g->n_tiles, h_out, [&](float* d) { return sp_adaptive_round(g, p, nullptr, d, stats, result); });
}

int sp_adaptive_tile_samples(sp_progress* g, uint32_t* h_out, int64_t capacity)
{
    if (!g || !h_out) return fail(SP_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lock(g->scene->mu);
    try {
        if (int rc = adaptive_object(g)) return rc;
        if (capacity < g->n_tiles) return fail(SP_ERR_ARG, "capacity below num_tiles");
        std::vector<uint32_t> done;
        if (int rc = adaptive_fetch(g, done, nullptr)) return rc;
        std::copy(done.begin(), done.end(), h_out);
        return SP_OK;
    } catch (const std::exception& e) {
        return fail(SP_ERR_HIP, std::string("sp_adaptive_tile_samples failed: ") + e.what());
    }
}

static int adaptive_tile_errors_impl(sp_progress* g, float floor, float* h_out, int64_t capacity)
{
    sp_scene* s = g->scene;
    if (int rc = adaptive_object(g)) return rc;
    if (!(floor >= 0.0f) || !std::isfinite(floor)) return fail(SP_ERR_ARG, "floor must be finite and >= 0");
    if (capacity < g->n_tiles) return fail(SP_ERR_ARG, "capacity below num_tiles");
    if (g->n_tiles == 0) return SP_OK;
    SP_HIP(hipSetDevice(s->device));
    if (int rc = wait_done(s)) return rc;
    spd::SelectArgs sa{};
    sa.tile_ids  = g->d_ids;
    sa.num_tiles = g->n_tiles;
    sa.tiles_x   = (g->width + 7) / 8;
    sa.width     = g->width;
    sa.height    = g->height;
    sa.floor     = floor == 0.0f ? 0.01f : floor;
    SP_HIP(spd::launch_adapt_select(g->ad, sa, g->ad.err, nullptr, nullptr)); // errors only: no selection
    SP_HIP(hipMemcpy(h_out, g->ad.err, (size_t)g->n_tiles * 4, hipMemcpyDeviceToHost));
    return SP_OK;
}

int sp_adaptive_tile_errors(sp_progress* g, float floor, float* h_out, int64_t capacity)
{
    if (!g || !h_out) return fail(SP_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lock(g->scene->mu);
    try {
        return adaptive_tile_errors_impl(g, floor, h_out, capacity);
    } catch (const std::exception& e) {
        return fail(SP_ERR_HIP, std::string("sp_adaptive_tile_errors failed: ") + e.what());
    }
}

static int adaptive_export_impl(sp_progress* g, sp_pixel_noise* h, int64_t capacity, uint32_t* h_tiles, int64_t tiles)
{
    if (int rc = adaptive_object(g)) return rc;
    const int64_t n_px = g->n_tiles * 64;
    if (capacity < n_px) return fail(SP_ERR_ARG, "capacity below num_tiles * 64 records");
    if (tiles < g->n_tiles) return fail(SP_ERR_ARG, "tiles below num_tiles");
    std::vector<uint32_t> done;
    if (int rc = adaptive_fetch(g, done, nullptr)) return rc;
    std::copy(done.begin(), done.end(), h_tiles);
    if (n_px == 0) return SP_OK;
    std::vector<float> mean((size_t)n_px), m2((size_t)n_px);
    SP_HIP(hipMemcpy(mean.data(), g->ad.mean, mean.size() * 4, hipMemcpyDeviceToHost));
    SP_HIP(hipMemcpy(m2.data(), g->ad.m2, m2.size() * 4, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n_px; ++i) h[i] = sp_pixel_noise{ mean[(size_t)i], m2[(size_t)i] };
    return SP_OK;
}

int sp_adaptive_export(sp_progress* g, sp_pixel_noise* h_noise, int64_t capacity, uint32_t* h_tile_samples, int64_t tiles)
{
    if (!g || !h_noise || !h_tile_samples) return fail(SP_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lock(g->scene->mu);
    try {
        return adaptive_export_impl(g, h_noise, capacity, h_tile_samples, tiles);
    } catch (const std::exception& e) {
        return fail(SP_ERR_HIP, std::string("sp_adaptive_export failed: ") + e.what());
    }
}

static int adaptive_import_impl(sp_progress* g, const sp_pixel_noise* h, int64_t count, const uint32_t* h_tiles, int64_t tiles)
{
    sp_scene* s = g->scene;
    if (int rc = adaptive_object(g)) return rc;
    const int64_t n_px = g->n_tiles * 64;
    if (count != n_px) return fail(SP_ERR_ARG, "count is not num_tiles * 64 records");
    if (tiles != g->n_tiles) return fail(SP_ERR_ARG, "tiles is not num_tiles");
    if (n_px == 0) return SP_OK;
    SP_HIP(hipSetDevice(s->device));
    if (int rc = wait_done(s)) return rc;
    std::vector<float> mean((size_t)n_px, 0.0f), m2((size_t)n_px, 0.0f);
    int32_t            x, y;
    for (int64_t i = 0; i < n_px; ++i) {
        if (!progress_pixel(g, i / 64, (uint32_t)(i % 64), x, y)) continue; // outside the image: stays zero
        mean[(size_t)i] = h[i].mean;
        m2[(size_t)i]   = h[i].m2;
    }
    uint32_t top = 0;
    for (int64_t i = 0; i < tiles; ++i) top = std::max(top, h_tiles[i]);
    SP_HIP(hipMemcpy(g->ad.mean, mean.data(), mean.size() * 4, hipMemcpyHostToDevice));
    SP_HIP(hipMemcpy(g->ad.m2, m2.data(), m2.size() * 4, hipMemcpyHostToDevice));
    SP_HIP(hipMemcpy(g->ad.done, h_tiles, (size_t)tiles * 4, hipMemcpyHostToDevice));
    g->st.n0 = top;
    return SP_OK;
}

int sp_adaptive_import(sp_progress* g, const sp_pixel_noise* h_noise, int64_t count, const uint32_t* h_tile_samples, int64_t tiles)
{
    if (!g || !h_noise || !h_tile_samples) return fail(SP_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lock(g->scene->mu);
    try {
        return adaptive_import_impl(g, h_noise, count, h_tile_samples, tiles);
    } catch (const std::exception& e) {
        return fail(SP_ERR_HIP, std::string("sp_adaptive_import failed: ") + e.what());
    }
}

int sp_tiles_to_image(int32_t width, int32_t height, const int32_t* tile_ids, int64_t num_tiles, const float* tiles,
                      float* image)
{
    if (!tiles || !image || width <= 0 || height <= 0) return fail(SP_ERR_ARG, "bad argument");
    int64_t total;
    sp_tile_count(width, height, &total);
    const int64_t n  = tile_ids ? num_tiles : total;
    const int32_t tw = (width + 7) / 8;
    for (int64_t sl = 0; sl < n; ++sl) {
        const int64_t t = tile_ids ? tile_ids[sl] : sl;
        if (t < 0 || t >= total) return fail(SP_ERR_ARG, "tile id out of range");
        const int32_t x0 = (int32_t)(t % tw) * 8, y0 = (int32_t)(t / tw) * 8;
        for (uint32_t m = 0; m < 64; ++m) {
            uint32_t a = m & 0x55u, b = (m >> 1) & 0x55u;
            a = (a | (a >> 1)) & 0x33u; a = (a | (a >> 2)) & 0x0fu;
            b = (b | (b >> 1)) & 0x33u; b = (b | (b >> 2)) & 0x0fu;
            const int32_t x = x0 + (int32_t)a, y = y0 + (int32_t)b;
            if (x >= width || y >= height) continue;
            for (int c = 0; c < 3; ++c) image[((size_t)y * width + x) * 3 + c] = tiles[((size_t)sl * 64 + m) * 3 + c];
        }
    }
    return SP_OK;
}

int sp_write_pfm(const char* path, int32_t width, int32_t height, const float* image)
{
    if (!path || !image) return fail(SP_ERR_ARG, "null argument");
    FILE* f = std::fopen(path, "wb");
    if (!f) return fail(SP_ERR_IO, std::string("Unable to open ") + path);
    std::fprintf(f, "PF\n%d %d\n%d\n", width, height, -1);
    for (int32_t j = height - 1; j >= 0; --j)
        std::fwrite(image + (size_t)j * width * 3, sizeof(float), (size_t)width * 3, f);
    std::fclose(f);
    return SP_OK;
}

// ---- what an upload would build (host only), and what a resident scene holds ------------------------

int sp_scene_bvh_build_info(const sp_scene* s, int32_t bvh_mode, sp_bvh_info* out)
{
    if (!s || !out) return fail(SP_ERR_ARG, "null argument");
    try {
        sp_upload_params up{}; // (resolve_opts refuses a bvh_mode that is neither 0 nor 1)
        up.bvh_mode = bvh_mode;
        UploadOpts opts;
        if (int rc = resolve_opts(&up, nullptr, UploadHooks::from_env(), opts)) return rc;
        HostAccel a;
        build_trees(*s->host, a, opts, BuildOn::HOST);
        std::vector<sph::PrimBounds>().swap(a.bounds);
        *out             = sp_bvh_info{};
        out->depth       = a.bvh.max_depth;
        out->nodes       = (int64_t)a.n_nodes;
        out->slots       = (int64_t)a.n_slots;
        out->light_depth = a.lbvh.max_depth;
        // the wide tree for its depth alone, no records (both collapses give the same tree)
        if (a.want_wide) out->wide_depth = sph::build_wide(a.bvh).depth;
        out->stack_depth = walk_plan(opts, out->depth, out->light_depth, out->wide_depth).stack_depth;
        return SP_OK;
    } catch (const std::exception& e) {
        return fail(SP_ERR_UNSUPPORTED, std::string("BVH build failed: ") + e.what());
    }
}

namespace {
// sp_bvh_check from the host checker's findings; bvh_mode 1 leaves are not limited (a failed split)
int fill_check(const sph::Bvh& bvh, const std::vector<sph::PrimBounds>& bounds, const UploadOpts& opts, sp_bvh_check* out)
{
    const sph::BvhCheck c = sph::check_bvh(bvh, bounds, opts.bvh_mode == 1 ? 0 : opts.sah_leaf);
    const uint32_t      sz = out->struct_size;
    *out                  = sp_bvh_check{};
    out->struct_size      = sz;
    out->builder          = opts.builder;
    out->nodes            = c.nodes;
    out->leaves           = c.leaves;
    out->slots            = c.slots;
    out->depth            = c.depth;
    out->max_leaf         = c.max_leaf;
    out->errors           = c.errors;
    out->first_error_kind = c.first_error_kind;
    out->first_error_node = c.first_error_node;
    out->hash             = c.hash;
    return SP_OK;
}

// sp_wide_check from the arrays a render reads
int fill_wide_check(const HostAccel& a, int finish, sp_wide_check* out)
{
    const uint32_t sz = out->struct_size;
    *out              = sp_wide_check{};
    out->struct_size  = sz;
    out->finish       = finish;
    if (!a.wide.words.empty()) {
        const sph::WideCheck c = sph::check_wide(a.wide, a.bvh.prim_order, a.bounds);
        out->records          = c.records;
        out->holes            = c.holes;
        out->slots            = c.slots;
        out->depth            = c.depth;
        out->errors           = c.errors;
        out->first_error_kind = c.first_error_kind;
        out->first_error_node = c.first_error_node;
        out->hash_nodes       = c.hash_nodes;
    }
    uint64_t h = sph::fnv1a64(a.slot_tri.data(), a.slot_tri.size() * sizeof(float4));
    h          = sph::fnv1a64(a.slot_code.data(), a.slot_code.size() * sizeof(uint32_t), h);
    out->hash_records = sph::fnv1a64(a.wslot_tri.data(), a.wslot_tri.size() * sizeof(float4), h);
    out->hash_parents = a.walk.stackless ? sph::fnv1a64(a.parents.data(), a.parents.size() * sizeof(uint32_t)) : 0;
    return SP_OK;
}

// slot -> index into `by` of the entry with that code; entries sharing a code (a scene may list a
// primitive twice) are handed out in order, -1 when none is left (the checkers report it)
void match_codes(const std::vector<uint32_t>& codes, const std::vector<uint32_t>& by, std::vector<int32_t>& out)
{
    std::vector<std::pair<uint32_t, int32_t>> by_code(by.size());
    for (size_t i = 0; i < by.size(); ++i) by_code[i] = { by[i], (int32_t)i };
    std::sort(by_code.begin(), by_code.end());
    std::vector<uint8_t> taken(by.size(), 0);
    out.assign(codes.size(), -1);
    for (size_t sl = 0; sl < codes.size(); ++sl) {
        auto it = std::lower_bound(by_code.begin(), by_code.end(), std::make_pair(codes[sl], (int32_t)0));
        while (it != by_code.end() && it->first == codes[sl] && taken[(size_t)(it - by_code.begin())]) ++it;
        if (it == by_code.end() || it->first != codes[sl]) continue;
        taken[(size_t)(it - by_code.begin())] = 1;
        out[sl] = it->second;
    }
}

// The resident scene's accelerators read back into `a`, as far as the checks look: bounds, the
// binary tree, its records (slot_code alone unless `finish`), and with `finish` the wide tree, its
// records and the parent links.  Each primitive's code (kind, index) names it: slot -> bounded
// primitive, and wide slot -> slot.
int download_accel(const sp_scene* s, HostAccel& a, bool finish)
{
    SP_HIP(hipSetDevice(s->device));
    SP_HIP(hipDeviceSynchronize()); // queued renders read these arrays; nothing writes them
    auto down = [&](auto& vec, const void* src) -> hipError_t {
        if (vec.empty()) return hipSuccess;
        if (!src) return hipErrorInvalidValue;
        return hipMemcpy(vec.data(), src, vec.size() * sizeof(vec[0]), hipMemcpyDeviceToHost);
    };
    const sph::Scene&    h  = *s->host;
    const spd::Scene&    d  = s->dev;
    const ResidentSizes& sz = s->sizes;
    a.bounds                = bounded_prims(h, a.prims, a.part);
    a.bvh.max_depth         = sz.geom_depth;
    a.bvh.nodes.resize(sz.geom_nodes);
    a.slot_code.resize(sz.geom_slots);
    SP_HIP(down(a.bvh.nodes, d.nodes));
    SP_HIP(down(a.slot_code, d.slot_code));
    std::vector<uint32_t> prim_codes(a.part);
    for (size_t i = 0; i < a.part; ++i) prim_codes[i] = code_of(h.prim_kind[a.prims[i]], h.prim_index[a.prims[i]]);
    match_codes(a.slot_code, prim_codes, a.bvh.prim_order);
    if (!finish) return SP_OK;
    a.walk.stackless = d.stackless != 0;
    a.slot_tri.resize(sz.geom_slots * 3);
    a.parents.resize(d.stackless ? sz.geom_nodes : 0);
    a.wslot_tri.resize(d.wnodes ? sz.wide_slots * 3 : 0);
    a.wide.words.resize(d.wnodes ? sz.wide_records * 20 : 0);
    a.wide.depth = d.wnodes ? sz.wide_depth : 0;
    SP_HIP(down(a.wide.words, d.wnodes));
    SP_HIP(down(a.slot_tri, d.slot_tri));
    SP_HIP(down(a.wslot_tri, d.wslot_tri));
    SP_HIP(down(a.parents, d.parents));
    std::vector<uint32_t> wcodes(a.wslot_tri.size() / 3);
    for (size_t i = 0; i < wcodes.size(); ++i) std::memcpy(&wcodes[i], &a.wslot_tri[3 * i].w, 4);
    match_codes(wcodes, a.slot_code, a.wide.slot_of);
    return SP_OK;
}

// The body of the four checks.  With `build`: what an upload with these options would make, on the
// host alone; without: the resident scene read back (the caller holds its lock).  Then the binary
// tree's check or, given `wide`, the finish's.
int check_scene(const sp_scene* s, const UploadOpts* build, sp_bvh_check* bvh, sp_wide_check* wide)
{
    const UploadOpts& opts = build ? *build : s->opts;
    try {
        HostAccel a;
        if (build) {
            build_trees(*s->host, a, opts, BuildOn::HOST);
            if (wide) finish_host(*s->host, a, opts);
        } else if (int rc = download_accel(s, a, wide != nullptr)) return rc;
        return wide ? fill_wide_check(a, opts.finish, wide) : fill_check(a.bvh, a.bounds, opts, bvh);
    } catch (const std::exception& e) { // a build keeps its own code; a read-back has none to keep
        const sph::SpError* se = build ? dynamic_cast<const sph::SpError*>(&e) : nullptr;
        if (se) return fail(se->code, e.what());
        return fail(SP_ERR_UNSUPPORTED, std::string(build ? "BVH build" : wide ? "wide BVH check" : "BVH check") + " failed: " + e.what());
    }
}
} // namespace

int sp_scene_bvh_build_check(const sp_scene* s, const sp_upload_params* params, const sp_build_params* build, sp_bvh_check* out)
{
    if (!s || !out) return fail(SP_ERR_ARG, "null argument");
    if (out->struct_size != sizeof(sp_bvh_check)) return fail(SP_ERR_ARG, "sp_bvh_check.struct_size is not a known size");
    UploadOpts opts;
    if (int rc = resolve_opts(params, build, UploadHooks::from_env(), opts)) return rc;
    return check_scene(s, &opts, out, nullptr);
}

int sp_scene_bvh_check(sp_scene* s, sp_bvh_check* out)
{
    if (!s || !out) return fail(SP_ERR_ARG, "null argument");
    if (out->struct_size != sizeof(sp_bvh_check)) return fail(SP_ERR_ARG, "sp_bvh_check.struct_size is not a known size");
    std::lock_guard<std::mutex> lock(s->mu);
    if (s->device < 0) return fail(SP_ERR_STATE, "scene not uploaded");
    return check_scene(s, nullptr, out, nullptr);
}

int sp_scene_wide_build_check(const sp_scene* s, const sp_upload_params* params, const sp_build_params* build, sp_wide_check* out)
{
    if (!s || !out) return fail(SP_ERR_ARG, "null argument");
    if (out->struct_size != sizeof(sp_wide_check)) return fail(SP_ERR_ARG, "sp_wide_check.struct_size is not a known size");
    UploadOpts opts;
    if (int rc = resolve_opts(params, build, UploadHooks::from_env(), opts)) return rc;
    return check_scene(s, &opts, nullptr, out);
}

int sp_scene_wide_check(sp_scene* s, sp_wide_check* out)
{
    if (!s || !out) return fail(SP_ERR_ARG, "null argument");
    if (out->struct_size != sizeof(sp_wide_check)) return fail(SP_ERR_ARG, "sp_wide_check.struct_size is not a known size");
    std::lock_guard<std::mutex> lock(s->mu);
    if (s->device < 0) return fail(SP_ERR_STATE, "scene not uploaded");
    return check_scene(s, nullptr, nullptr, out);
}

// ---- moving meshes: refit ------------------------------------------------------------

namespace {
// sp_mesh_update against the scene's mesh, in the order the header promises (the scene itself is the
// caller's): struct size, reserved fields, null vertices, the vertex count.  Changes nothing.
int validate_update(const sph::Scene& h, const sp_mesh_update* u)
{
    if (!u) return fail(SP_ERR_ARG, "null sp_mesh_update");
    if (u->struct_size != sizeof(sp_mesh_update)) return fail(SP_ERR_ARG, "sp_mesh_update.struct_size is not a known size");
    if (u->reserved0 != 0 || u->reserved[0] != 0 || u->reserved[1] != 0 || u->reserved[2] != 0 || u->reserved[3] != 0)
        return fail(SP_ERR_ARG, "sp_mesh_update.reserved must be 0");
    if (!u->vertices && !(h.vertices.empty() && u->num_vertices == 0)) return fail(SP_ERR_ARG, "sp_mesh_update.vertices is null");
    if (u->num_vertices != (int64_t)h.vertices.size()) return fail(SP_ERR_ARG, "sp_mesh_update.num_vertices is not the scene's");
    return SP_OK;
}

void copy_f3(std::vector<spm::f3>& to, const float* from)
{
    static_assert(sizeof(spm::f3) == 12, "f3 packing");
    if (!to.empty()) std::memcpy(to.data(), from, to.size() * sizeof(spm::f3));
}

// what bounded_prims and pack_records read of a scene, with other vertex positions
sph::Scene moved_mesh(const sph::Scene& h, const float* vertices)
{
    sph::Scene m;
    m.vertices   = h.vertices;
    m.indices    = h.indices;
    m.shapes     = h.shapes;
    m.prim_kind  = h.prim_kind;
    m.prim_index = h.prim_index;
    copy_f3(m.vertices, vertices);
    return m;
}

// The host restatement of the device refit (sp_refit.hip) on the arrays finish_host made: the
// records again from the moved mesh, every binary box by lbvh_fit_boxes, every wide record by
// refit_wide.  Topology, prim_order and slot_of stay; a.bounds become the new bounds.
void refit_host(HostAccel& a, const sph::Scene& moved)
{
    a.bounds = bounded_prims(moved, a.prims, a.part);
    pack_records(moved, a.prims, a.bvh.prim_order, a.slot_tri, a.slot_code);
    for (size_t i = 0; i < a.wide.slot_of.size(); ++i)
        for (int k = 0; k < 3; ++k) a.wslot_tri[3 * i + k] = a.slot_tri[3 * (size_t)a.wide.slot_of[i] + k];
    sph::lbvh_fit_boxes(a.bvh, a.bounds);
    if (a.wide.words.empty()) return;
    std::vector<sph::PrimBounds> by_wide_slot(a.wide.slot_of.size());
    for (size_t i = 0; i < by_wide_slot.size(); ++i)
        by_wide_slot[i] = a.bounds[(size_t)a.bvh.prim_order[(size_t)a.wide.slot_of[i]]];
    sph::refit_wide(a.wide, by_wide_slot);
}

// bounds by shape index for the device: the host's sphere_bounds values (a plane has none)
std::vector<sph::PrimBounds> shape_bounds(const sph::Scene& h)
{
    std::vector<sph::PrimBounds> out(h.shapes.size());
    for (size_t i = 0; i < out.size(); ++i) {
        if (h.shapes[i].kind == SP_PRIM_SPHERE) out[i] = sphere_bounds(from_desc(h.shapes[i].object_to_world));
        else
            for (int d = 0; d < 3; ++d) { out[i].lo[d] = INFINITY; out[i].hi[d] = -INFINITY; }
    }
    return out;
}

// the resident arrays follow the host mesh (already the new one); the caller holds the lock
int refit_resident(sp_scene* s, bool with_normals, bool timed, spr::RefitStats& st)
{
    const sph::Scene& h = *s->host;
    const spd::Scene& d = s->dev;
    SP_HIP(hipSetDevice(s->device));
    SP_HIP(hipDeviceSynchronize()); // queued renders read the arrays this rewrites
    const std::vector<sph::PrimBounds> shapes = shape_bounds(h);
    spr::RefitIn in;
    in.d_nodes     = reinterpret_cast<sph::BvhNode*>(const_cast<spd::Node*>(d.nodes));
    in.n_nodes     = (uint32_t)s->sizes.geom_nodes;
    in.geom_depth  = s->sizes.geom_depth;
    in.d_slot_tri  = const_cast<float4*>(d.slot_tri);
    in.d_slot_code = d.slot_code;
    in.n_slots     = (uint32_t)s->sizes.geom_slots;
    if (d.wnodes) {
        in.d_wnodes    = reinterpret_cast<uint32_t*>(const_cast<uint4*>(d.wnodes));
        in.records     = (uint32_t)s->sizes.wide_records;
        in.wide_depth  = s->sizes.wide_depth;
        in.d_wslot_tri = const_cast<float4*>(d.wslot_tri);
        in.wide_slots  = (uint32_t)s->sizes.wide_slots;
    }
    in.d_indices      = d.indices;
    in.n_indices      = h.indices.size();
    in.h_verts        = h.vertices.data();
    in.n_verts        = h.vertices.size();
    in.h_normals      = with_normals ? h.normals.data() : nullptr;
    in.d_normals      = const_cast<float*>(d.normals);
    in.h_shape_bounds = shapes.data();
    in.n_shapes       = (uint32_t)shapes.size();
    std::string err;
    const int   rc = spr::refit_device(in, st, err, timed);
    return rc == SP_OK ? SP_OK : fail(rc, err);
}
} // namespace

int sp_scene_update_mesh(sp_scene* s, const sp_mesh_update* u, sp_refit_stats* stats)
{
    if (!s) return fail(SP_ERR_ARG, "null scene");
    if (stats && stats->struct_size != sizeof(sp_refit_stats)) return fail(SP_ERR_ARG, "sp_refit_stats.struct_size is not a known size");
    std::lock_guard<std::mutex> lock(s->mu);
    sph::Scene&                 h = *s->host;
    if (int rc = validate_update(h, u)) return rc;
    if (s->device >= 0 && s->opts.bvh_mode == 1)
        return fail(SP_ERR_ARG, "a scene resident in the reference order (bvh_mode 1) cannot be refitted: upload it again");
    if (stats) {
        *stats             = sp_refit_stats{};
        stats->struct_size = sizeof(sp_refit_stats);
    }
    if (h.vertices.empty()) return SP_OK;
    copy_f3(h.vertices, u->vertices);
    if (u->normals && h.normals.size() == h.vertices.size()) copy_f3(h.normals, u->normals);
    if (s->device < 0) return SP_OK;
    const bool      env_timing = UploadHooks::from_env().timing;
    spr::RefitStats st;
    int             rc = SP_OK;
    ++s->generation; // the samples of every progress object belong to the old geometry
    try {
        rc = refit_resident(s, u->normals != nullptr && h.normals.size() == h.vertices.size(), stats != nullptr || env_timing, st);
    } catch (const std::exception& e) {
        rc = fail(SP_ERR_UNSUPPORTED, std::string("mesh update failed: ") + e.what());
    }
    if (rc != SP_OK) {
        (void)hipGetLastError();
        s->release(); // as after a failed upload: no resident scene; the host mesh is the new one
        return rc;
    }
    s->refitted = true;
    if (stats) {
        stats->refitted      = 1;
        stats->binary_passes = st.binary_passes;
        stats->wide_passes   = st.wide_passes;
        stats->ms_copy       = (float)st.ms_copy;
        stats->ms_pack       = (float)st.ms_pack;
        stats->ms_binary     = (float)st.ms_binary;
        stats->ms_wide       = (float)st.ms_wide;
        stats->ms_total      = (float)st.ms_total;
        stats->scratch_bytes = (int64_t)st.peak_bytes;
    }
    if (env_timing)
        std::fprintf(stderr,
                     "sp_refit_timing {\"nodes\": %zu, \"slots\": %zu, \"records\": %zu, \"binary_passes\": %d, \"wide_passes\": %d, "
                     "\"copy_ms\": %.3f, \"pack_ms\": %.3f, \"binary_ms\": %.3f, \"wide_ms\": %.3f, \"total_ms\": %.3f, "
                     "\"peak_scratch_bytes\": %zu}\n",
                     s->sizes.geom_nodes, s->sizes.geom_slots, s->sizes.wide_records, st.binary_passes, st.wide_passes, st.ms_copy,
                     st.ms_pack, st.ms_binary, st.ms_wide, st.ms_total, st.peak_bytes);
    return SP_OK;
}

int sp_scene_refit_build_check(const sp_scene* s, const sp_upload_params* params, const sp_build_params* build,
                               const sp_mesh_update* u, sp_bvh_check* bvh, sp_wide_check* wide)
{
    if (!s) return fail(SP_ERR_ARG, "null scene");
    if (bvh && bvh->struct_size != sizeof(sp_bvh_check)) return fail(SP_ERR_ARG, "sp_bvh_check.struct_size is not a known size");
    if (wide && wide->struct_size != sizeof(sp_wide_check)) return fail(SP_ERR_ARG, "sp_wide_check.struct_size is not a known size");
    if (int rc = validate_update(*s->host, u)) return rc;
    UploadOpts opts;
    if (int rc = resolve_opts(params, build, UploadHooks::from_env(), opts)) return rc;
    if (opts.bvh_mode == 1) return fail(SP_ERR_ARG, "the reference order (bvh_mode 1) is not refitted");
    try {
        HostAccel a;
        build_trees(*s->host, a, opts, BuildOn::HOST);
        finish_host(*s->host, a, opts);
        refit_host(a, moved_mesh(*s->host, u->vertices));
        if (bvh) fill_check(a.bvh, a.bounds, opts, bvh);
        if (wide) fill_wide_check(a, opts.finish, wide);
        return SP_OK;
    } catch (const sph::SpError& e) {
        return fail(e.code, e.what());
    } catch (const std::exception& e) {
        return fail(SP_ERR_UNSUPPORTED, std::string("refit check failed: ") + e.what());
    }
}

// ---- relighting: material, light and sky edits ---------------------------------------

namespace {
#define SP_TRY(call) do { if (int rc__ = (call)) return rc__; } while (0)

// the start of every edit of a resident scene (the caller holds the lock): nothing queued reads the
// arrays any more, and every progress object made on the scene is retired
int begin_edit(sp_scene* s)
{
    SP_HIP(hipSetDevice(s->device));
    SP_TRY(wait_done(s));
    ++s->generation;
    return SP_OK;
}

// how an edit ends: a failure leaves no resident scene, as after a failed upload
int end_edit(sp_scene* s, int rc)
{
    if (rc == SP_OK) return SP_OK;
    (void)hipGetLastError();
    s->release();
    return rc;
}

spm::lin lin_of(const sp_linear& d) { return from_desc(d); }
bool     same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

// sp_env_update against the scene, in the order the header promises; changes nothing
int validate_env_update(const sp_scene* s, const sp_env_update* u, const sp_env_stats* stats)
{
    if (!u) return fail(SP_ERR_ARG, "null sp_env_update");
    if (u->struct_size != sizeof(sp_env_update)) return fail(SP_ERR_ARG, "sp_env_update.struct_size is not a known size");
    if (stats && stats->struct_size != sizeof(sp_env_stats)) return fail(SP_ERR_ARG, "sp_env_stats.struct_size is not a known size");
    if (u->reserved0 != 0 || u->reserved[0] != 0 || u->reserved[1] != 0 || u->reserved[2] != 0 || u->reserved[3] != 0)
        return fail(SP_ERR_ARG, "sp_env_update.reserved must be 0");
    const int32_t n = (int32_t)s->host->env_images.size();
    if (u->image < 0 || u->image > n) return fail(SP_ERR_ARG, "sp_env_update.image is out of range");
    if (u->pixels && u->d_pixels) return fail(SP_ERR_ARG, "sp_env_update: pixels and d_pixels are both given");
    if (u->pixels || u->d_pixels) {
        if (u->width < 1 || u->height < 1 || u->width > 32767 || u->height > 32767)
            return fail(SP_ERR_ARG, "sp_env_update: bad image size");
    } else {
        if (u->image == n) return fail(SP_ERR_ARG, "sp_env_update: an appended image needs pixels");
        const sph::EnvImage& e = s->host->env_images[(size_t)u->image];
        if (!((u->width == 0 && u->height == 0) || (u->width == e.width && u->height == e.height)))
            return fail(SP_ERR_ARG, "sp_env_update: without pixels the size is 0 or the current one");
    }
    if (u->d_pixels && s->device < 0) return fail(SP_ERR_STATE, "sp_env_update.d_pixels needs a resident scene");
    return SP_OK;
}

void fill_env_stats(sp_env_stats* stats, int rebuilt, bool guided, const spe::EnvBuildStats& st)
{
    if (!stats) return;
    *stats             = sp_env_stats{};
    stats->struct_size = sizeof(sp_env_stats);
    stats->rebuilt     = rebuilt;
    stats->guided      = guided ? 1 : 0;
    stats->ms_upload   = (float)st.ms_upload;
    stats->ms_clamp    = (float)st.ms_clamp;
    stats->ms_func     = (float)st.ms_func;
    stats->ms_rows     = (float)st.ms_rows;
    stats->ms_marginal = (float)st.ms_marginal;
    stats->ms_guides   = (float)st.ms_guides;
    stats->ms_total    = (float)st.ms_total;
    stats->scratch_bytes = (int64_t)st.peak_bytes;
}

// the resident side of sp_scene_set_env_image; the host scene is the edited one already
int relight_env(sp_scene* s, size_t i, const float* d_pixels, bool matrices_only, sp_env_stats* stats)
{
    spe::EnvBuildStats st;
    if (matrices_only) {
        const sph::EnvImage& e = s->host->env_images[i];
        s->env_recs[i].l2w     = e.light_to_world;
        s->env_recs[i].w2l     = e.world_to_light;
        SP_HIP(hipMemcpy(s->env_recs_buf.as<spd::EnvMap>() + i, &s->env_recs[i], sizeof(spd::EnvMap), hipMemcpyHostToDevice));
        fill_env_stats(stats, 0, s->env_blocks[i].guided, st);
        return SP_OK;
    }
    if (i == s->env_blocks.size()) {
        s->env_blocks.emplace_back();
        s->env_recs.emplace_back();
    }
    SP_TRY(env_build_device(s, i, d_pixels, s->opts.env_guide, st, stats != nullptr));
    SP_TRY(upload_env_records(s));
    fill_env_stats(stats, 1, s->env_blocks[i].guided, st);
    return SP_OK;
}

// FNV-1a 64 of a table (0: absent)
uint64_t table_hash(const void* p, size_t bytes) { return bytes ? sph::fnv1a64(p, bytes) : 0; }

struct EnvTables { // one map's tables as words, in SP_ENV_* order
    std::vector<uint32_t> t[SP_ENV_TABLES];
    bool                  guided = false;
    uint32_t              marg_int_bits = 0;
};

EnvTables host_tables(const sph::EnvImage& e)
{
    const sph::EnvMap m = sph::build_env_map(e);
    EnvTables         x;
    auto              to_words = [](const auto& v, std::vector<uint32_t>& w) {
        static_assert(sizeof(v[0]) == 4, "a table of words");
        w.resize(v.size());
        if (!v.empty()) std::memcpy(w.data(), v.data(), v.size() * 4);
    };
    x.t[SP_ENV_RADIANCE].assign((size_t)m.w * m.h * 4, 0u);
    for (size_t k = 0; k < (size_t)m.w * m.h; ++k) std::memcpy(&x.t[SP_ENV_RADIANCE][4 * k], &m.radiance[3 * k], 12);
    to_words(m.cond_func, x.t[SP_ENV_COND_FUNC]);
    to_words(m.cond_cdf, x.t[SP_ENV_COND_CDF]);
    to_words(m.cond_int, x.t[SP_ENV_COND_INT]);
    to_words(m.marg_func, x.t[SP_ENV_MARG_FUNC]);
    to_words(m.marg_cdf, x.t[SP_ENV_MARG_CDF]);
    to_words(m.cond_guide, x.t[SP_ENV_COND_GUIDE]);
    to_words(m.marg_guide, x.t[SP_ENV_MARG_GUIDE]);
    x.guided = m.guided;
    std::memcpy(&x.marg_int_bits, &m.marg_int, 4);
    return x;
}

void fill_env_check(sp_env_check* out, const sph::EnvImage& e, const EnvTables& x, int builder)
{
    const spe::EnvSizes z = spe::env_sizes(e.width, e.height);
    *out               = sp_env_check{};
    out->struct_size   = sizeof(sp_env_check);
    out->builder       = builder;
    out->width         = e.width;
    out->height        = e.height;
    out->nu            = z.nu;
    out->nv            = z.nv;
    out->guided        = x.guided ? 1 : 0;
    out->cond_bits     = z.cond_bits;
    out->marg_bits     = z.marg_bits;
    out->marg_int_bits = x.marg_int_bits;
    out->first_table   = -1;
    out->first_index   = -1;
    for (int k = 0; k < SP_ENV_TABLES; ++k) out->hash[k] = table_hash(x.t[k].data(), x.t[k].size() * 4);
}
} // namespace

int sp_scene_set_materials(sp_scene* s, const sp_material_desc* materials, int32_t num_materials)
{
    if (!s) return fail(SP_ERR_ARG, "null scene");
    std::lock_guard<std::mutex> lock(s->mu);
    sph::Scene&                 h = *s->host;
    if (!materials && num_materials != 0) return fail(SP_ERR_ARG, "sp_scene_set_materials: null materials");
    if (num_materials != (int32_t)h.materials.size()) return fail(SP_ERR_ARG, "sp_scene_set_materials: num_materials is not the scene's");
    for (int32_t i = 0; i < num_materials; ++i) {
        const sp_material_desc& m = materials[i];
        if (m.kind < SP_MAT_LAMBERTIAN || m.kind > SP_MAT_CLEARCOAT ||
            (m.kind == SP_MAT_CLEARCOAT && (m.base < 0 || m.base >= num_materials)))
            return fail(SP_ERR_ARG, "sp_scene_set_materials: bad material");
    }
    for (int32_t i = 0; i < num_materials; ++i)
        if (materials[i].kind == SP_MAT_CLEARCOAT && materials[materials[i].base].kind == SP_MAT_CLEARCOAT)
            return fail(SP_ERR_UNSUPPORTED, "clearcoat over clearcoat");
    try {
        for (int32_t i = 0; i < num_materials; ++i) h.materials[(size_t)i].d = materials[i];
        fill_desc(s);
        if (s->device < 0 || num_materials == 0) return SP_OK;
        std::vector<spd::Material> mats;
        SP_TRY(convert_materials(h, mats));
        int rc = begin_edit(s);
        if (rc == SP_OK) {
            const hipError_t e = hipMemcpy(const_cast<spd::Material*>(s->dev.materials), mats.data(), mats.size() * sizeof(spd::Material),
                                           hipMemcpyHostToDevice);
            if (e != hipSuccess) rc = fail(SP_ERR_HIP, std::string("sp_scene_set_materials: ") + hipGetErrorString(e));
        }
        return end_edit(s, rc);
    } catch (const std::exception& e) {
        return end_edit(s, fail(SP_ERR_UNSUPPORTED, std::string("sp_scene_set_materials: ") + e.what()));
    }
}

int sp_scene_set_lights(sp_scene* s, const sp_light_desc* lights, int32_t num_lights)
{
    if (!s) return fail(SP_ERR_ARG, "null scene");
    std::lock_guard<std::mutex> lock(s->mu);
    sph::Scene&                 h = *s->host;
    if (num_lights < 0) return fail(SP_ERR_ARG, "sp_scene_set_lights: num_lights < 0");
    if (!lights && num_lights != 0) return fail(SP_ERR_ARG, "sp_scene_set_lights: null lights");
    for (int32_t i = 0; i < num_lights; ++i) {
        const sp_light_desc& l = lights[i];
        if (l.kind < SP_LIGHT_SPHERE || l.kind > SP_LIGHT_IMAGE_ENVIRONMENT) return fail(SP_ERR_ARG, "sp_scene_set_lights: bad light kind");
        if (l.kind == SP_LIGHT_IMAGE_ENVIRONMENT && (l.image < 0 || l.image >= (int32_t)h.env_images.size()))
            return fail(SP_ERR_ARG, "sp_scene_set_lights: light image out of range");
    }
    try {
        std::vector<sp_light_desc> list(lights, lights + num_lights);
        HostAccel                  a;
        WalkPlan                   walk;
        if (s->device >= 0) { // the new accelerator first: a walk that cannot follow is refused before anything changes
            build_light_tree(list, a);
            walk = walk_plan(s->opts, s->sizes.geom_depth, a.lbvh.max_depth, s->sizes.wide_depth);
            if (walk.stackless != (s->dev.stackless != 0))
                return fail(SP_ERR_UNSUPPORTED, "sp_scene_set_lights: the light BVH's depth changes how the resident scene is walked: upload again");
            if (walk.stackless) a.light_parents = parent_links(a.lbvh.nodes);
        }
        h.lights.swap(list);
        fill_desc(s);
        if (s->device < 0) return SP_OK;
        int rc = begin_edit(s);
        if (rc == SP_OK) rc = upload_lights(s, a);
        if (rc == SP_OK) {
            s->sizes.light_depth = a.lbvh.max_depth;
            apply_walk_plan(s, s->opts, walk);
        }
        return end_edit(s, rc);
    } catch (const std::exception& e) {
        return end_edit(s, fail(SP_ERR_UNSUPPORTED, std::string("sp_scene_set_lights: ") + e.what()));
    }
}

int sp_scene_set_env_image(sp_scene* s, const sp_env_update* u, sp_env_stats* stats)
{
    if (!s) return fail(SP_ERR_ARG, "null scene");
    std::lock_guard<std::mutex> lock(s->mu);
    SP_TRY(validate_env_update(s, u, stats));
    sph::Scene& h = *s->host;
    try {
        const size_t i        = (size_t)u->image;
        const bool   pixels   = u->pixels || u->d_pixels;
        const bool   matrices = !pixels && same_bits(u->max_radiance, h.env_images[i].max_radiance);
        if (i == h.env_images.size()) h.env_images.emplace_back();
        sph::EnvImage& e = h.env_images[i];
        if (pixels) {
            const size_t n = (size_t)u->width * (size_t)u->height * 3;
            if (u->pixels) {
                std::vector<float> px(u->pixels, u->pixels + n); // (a copy first: `pixels` may be the scene's own)
                e.pixels.swap(px);
            } else {
                // the device copy comes back so that the host scene stays the truth
                std::vector<float> px(n);
                hipError_t         err = hipSetDevice(s->device);
                if (err == hipSuccess) err = hipMemcpy(px.data(), u->d_pixels, n * sizeof(float), hipMemcpyDeviceToHost);
                if (err != hipSuccess) {
                    (void)hipGetLastError();
                    if (i + 1 == h.env_images.size() && e.pixels.empty()) h.env_images.pop_back(); // (an append that never was)
                    return fail(SP_ERR_HIP, std::string("sp_scene_set_env_image: d_pixels: ") + hipGetErrorString(err));
                }
                e.pixels.swap(px);
            }
            e.width  = u->width;
            e.height = u->height;
        }
        e.max_radiance   = u->max_radiance;
        e.light_to_world = lin_of(u->light_to_world);
        e.world_to_light = lin_of(u->world_to_light);
        fill_desc(s);
        if (s->device < 0) {
            fill_env_stats(stats, 0, false, spe::EnvBuildStats{});
            return SP_OK;
        }
        int rc = begin_edit(s);
        if (rc == SP_OK) rc = relight_env(s, i, static_cast<const float*>(u->d_pixels), matrices, stats);
        return end_edit(s, rc);
    } catch (const std::exception& e) {
        return end_edit(s, fail(SP_ERR_UNSUPPORTED, std::string("sp_scene_set_env_image: ") + e.what()));
    }
}

int sp_scene_env_build_check(const sp_scene* s, int32_t image, sp_env_check* out)
{
    if (!s || !out) return fail(SP_ERR_ARG, "null argument");
    if (out->struct_size != sizeof(sp_env_check)) return fail(SP_ERR_ARG, "sp_env_check.struct_size is not a known size");
    if (image < 0 || image >= (int32_t)s->host->env_images.size()) return fail(SP_ERR_ARG, "env image out of range");
    try {
        const sph::EnvImage& e = s->host->env_images[(size_t)image];
        fill_env_check(out, e, host_tables(e), SP_ENV_BUILDER_HOST);
        return SP_OK;
    } catch (const std::exception& e) {
        return fail(SP_ERR_UNSUPPORTED, std::string("env build check failed: ") + e.what());
    }
}

int sp_scene_env_check(sp_scene* s, int32_t image, sp_env_check* out)
{
    if (!s || !out) return fail(SP_ERR_ARG, "null argument");
    if (out->struct_size != sizeof(sp_env_check)) return fail(SP_ERR_ARG, "sp_env_check.struct_size is not a known size");
    std::lock_guard<std::mutex> lock(s->mu);
    if (image < 0 || image >= (int32_t)s->host->env_images.size()) return fail(SP_ERR_ARG, "env image out of range");
    if (s->device < 0) return fail(SP_ERR_STATE, "scene not uploaded");
    try {
        const sph::EnvImage& e    = s->host->env_images[(size_t)image];
        const EnvTables      host = host_tables(e);
        const EnvBlocks&     b    = s->env_blocks[(size_t)image];
        const spd::EnvMap&   r    = s->env_recs[(size_t)image];
        SP_HIP(hipSetDevice(s->device));
        SP_HIP(hipDeviceSynchronize());
        EnvTables            dev;
        const DeviceScratch* blocks[SP_ENV_TABLES] = { &b.radiance, &b.cond_func, &b.cond_cdf, &b.cond_int,
                                                       &b.marg_func, &b.marg_cdf, &b.cond_guide, &b.marg_guide };
        for (int k = 0; k < SP_ENV_TABLES; ++k) {
            dev.t[k].resize(blocks[k]->cap / 4);
            if (blocks[k]->cap) SP_HIP(hipMemcpy(dev.t[k].data(), blocks[k]->ptr, blocks[k]->cap, hipMemcpyDeviceToHost));
        }
        dev.guided = b.guided;
        std::memcpy(&dev.marg_int_bits, &r.marg_int, 4);
        fill_env_check(out, e, dev, b.builder);
        auto miss = [&](int table, int64_t index) {
            if (out->mismatches++ == 0) {
                out->first_table = table;
                out->first_index = index;
            }
        };
        for (int k = 0; k < SP_ENV_TABLES; ++k) {
            const bool guide = k == SP_ENV_COND_GUIDE || k == SP_ENV_MARG_GUIDE;
            if (guide && !(host.guided && s->opts.env_guide)) { // env_replay, or unguided: the resident scene holds no guides
                if (!dev.t[k].empty()) miss(k, 0);
                continue;
            }
            if (dev.t[k].size() != host.t[k].size()) {
                miss(k, (int64_t)std::min(dev.t[k].size(), host.t[k].size()));
                continue;
            }
            for (size_t w = 0; w < dev.t[k].size(); ++w)
                if (dev.t[k][w] != host.t[k][w]) miss(k, (int64_t)w);
        }
        if (dev.guided != host.guided) miss(SP_ENV_SCALARS, 0);
        if (dev.marg_int_bits != host.marg_int_bits) miss(SP_ENV_SCALARS, 1);
        if (r.w != e.width || r.h != e.height || r.nu != out->nu || r.nv != out->nv) miss(SP_ENV_SCALARS, 2);
        if (r.cond_bits != out->cond_bits || r.marg_bits != out->marg_bits) miss(SP_ENV_SCALARS, 3);
        return SP_OK;
    } catch (const std::exception& e) {
        return fail(SP_ERR_UNSUPPORTED, std::string("env check failed: ") + e.what());
    }
}
#undef SP_TRY

// ---- ray queries (sp_query.hip) -----------------------------------------------------------------

// Everything sp_scene_trace_rays refuses, in the header's order; changes nothing.  The scene's
// lock is held (s->device is read last).  device_pointers: the alignment rules of device buffers
// (the host form asks none of its host arrays).
static int validate_query(const sp_scene* s, const sp_ray_query* q, const sp_ray_query_stats* stats, bool device_pointers)
{
    if (q->struct_size != sizeof(sp_ray_query)) return fail(SP_ERR_ARG, "sp_ray_query.struct_size is not this library's");
    if (stats && stats->struct_size != sizeof(sp_ray_query_stats))
        return fail(SP_ERR_ARG, "sp_ray_query_stats.struct_size is not this library's");
    for (int32_t r : q->reserved)
        if (r != 0) return fail(SP_ERR_ARG, "sp_ray_query.reserved must be 0");
    if (q->mode != SP_QUERY_CLOSEST && q->mode != SP_QUERY_ANY) return fail(SP_ERR_ARG, "unknown query mode");
    if (q->num_rays < 0) return fail(SP_ERR_ARG, "num_rays < 0");
    const bool any = q->mode == SP_QUERY_ANY;
    if (any && (q->d_hits || q->d_normals)) return fail(SP_ERR_ARG, "SP_QUERY_ANY: d_hits and d_normals must be NULL");
    if (!any && q->d_occluded) return fail(SP_ERR_ARG, "SP_QUERY_CLOSEST: d_occluded must be NULL");
    if (q->num_rays > 0) {
        if (!q->d_rays) return fail(SP_ERR_ARG, "d_rays is NULL");
        if (any && !q->d_occluded) return fail(SP_ERR_ARG, "SP_QUERY_ANY needs d_occluded");
        if (!any && !q->d_hits) return fail(SP_ERR_ARG, "SP_QUERY_CLOSEST needs d_hits");
    }
    if (device_pointers) {
        const auto off = [](const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
        if (off(q->d_rays, 16) || off(q->d_hits, 16) || off(q->d_normals, 16))
            return fail(SP_ERR_ARG, "d_rays, d_hits and d_normals must be 16-byte aligned");
        if (off(q->d_occluded, 4)) return fail(SP_ERR_ARG, "d_occluded must be 4-byte aligned");
    }
    if (s->device < 0) return fail(SP_ERR_STATE, "sp_scene_upload must be called before sp_scene_trace_rays");
    return SP_OK;
}

static int trace_rays_impl(sp_scene* s, const sp_ray_query* q, sp_ray_query_stats* stats)
{
    if (int rc = validate_query(s, q, stats, true)) return rc;
    const bool any = q->mode == SP_QUERY_ANY;
    if (stats) {
        *stats             = sp_ray_query_stats{};
        stats->struct_size = sizeof(sp_ray_query_stats);
        stats->stack_depth = any ? s->dev.any_stack_words : s->dev.stack_words;
    }
    if (q->num_rays == 0) return SP_OK;
    if (q->num_rays > ((int64_t)1 << 39) - spd::QUERY_BLOCK) return fail(SP_ERR_UNSUPPORTED, "more rays than one launch takes");
    const size_t lds_bytes = spd::query_lds_bytes(s->dev, any, q->d_normals != nullptr);
    if (lds_bytes > 160 * 1024) return fail(SP_ERR_UNSUPPORTED, "BVH too deep for the LDS traversal stack");
    SP_HIP(hipSetDevice(s->device));
    RenderScratch& r      = s->scratch;
    hipStream_t    stream = static_cast<hipStream_t>(q->stream);
    // the previous call on this scene (a render, a refit's successor, another query) comes first
    if (r.done_rec) SP_HIP(hipStreamWaitEvent(stream, r.ev_done, 0));
    spd::QueryArgs a{};
    a.rays     = q->d_rays;
    a.num_rays = q->num_rays;
    a.hits     = q->d_hits;
    a.normals  = reinterpret_cast<float4*>(q->d_normals);
    a.occluded = q->d_occluded;
    if (stats) { // counted only when asked for: word 5 of the render counters, which every call clears for itself
        a.hit_count = r.counters.as<unsigned long long>() + 5;
        SP_HIP(hipMemsetAsync(a.hit_count, 0, sizeof(unsigned long long), stream));
    }
    SP_HIP(hipEventRecord(r.ev0, stream));
    SP_HIP(any ? spd::launch_query_any(s->dev, a, lds_bytes, stream) : spd::launch_query_closest(s->dev, a, lds_bytes, stream));
    if (int rc = end_call(s, stream)) return rc;
    if (!stats) return SP_OK; // stream order: the query is only enqueued
    SP_HIP(hipEventSynchronize(r.ev1));
    unsigned long long hits = 0;
    SP_HIP(hipMemcpy(&hits, a.hit_count, sizeof(hits), hipMemcpyDeviceToHost));
    SP_HIP(hipEventElapsedTime(&stats->kernel_ms, r.ev0, r.ev1));
    stats->launches = 1;
    stats->rays     = (uint64_t)q->num_rays;
    stats->hits     = hits;
    return SP_OK;
}

int sp_scene_trace_rays(sp_scene* s, const sp_ray_query* q, sp_ray_query_stats* stats)
{
    if (!s || !q) return fail(SP_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lock(s->mu); // calls on one scene run one at a time (sp_scene::mu)
    try {
        return trace_rays_impl(s, q, stats);
    } catch (const std::exception& e) {
        return fail(SP_ERR_HIP, std::string("ray query failed: ") + e.what());
    }
}

// the host form with the scene's lock held: the same refusals in the same order on the host
// arrays as given, then device buffers of its own around the device form
static int trace_rays_host_impl(sp_scene* s, int32_t mode, const sp_ray* h_rays, int64_t num_rays, sp_ray_hit* h_hits,
                                float* h_normals, uint32_t* h_occluded, sp_ray_query_stats* stats)
{
    sp_ray_query q{};
    q.struct_size = sizeof(q);
    q.mode        = mode;
    q.d_rays      = h_rays;
    q.num_rays    = num_rays;
    q.d_hits      = h_hits;
    q.d_normals   = h_normals;
    q.d_occluded  = h_occluded;
    if (int rc = validate_query(s, &q, stats, false)) return rc;
    SP_HIP(hipSetDevice(s->device));
    const size_t  n = (size_t)num_rays;
    DeviceScratch d_rays, d_hits, d_normals, d_occ;
    const auto    device_copy = [](DeviceScratch& d, const void* host, size_t bytes) -> int {
        if (host) SP_HIP(d.reserve(std::max<size_t>(bytes, 16)));
        return SP_OK;
    };
    if (int rc = device_copy(d_rays, h_rays, n * sizeof(sp_ray))) return rc;
    if (int rc = device_copy(d_hits, h_hits, n * sizeof(sp_ray_hit))) return rc;
    if (int rc = device_copy(d_normals, h_normals, n * 4 * sizeof(float))) return rc;
    if (int rc = device_copy(d_occ, h_occluded, n * sizeof(uint32_t))) return rc;
    if (n) SP_HIP(hipMemcpy(d_rays.ptr, h_rays, n * sizeof(sp_ray), hipMemcpyHostToDevice));
    q.d_rays     = d_rays.as<sp_ray>();
    q.d_hits     = d_hits.as<sp_ray_hit>();
    q.d_normals  = d_normals.as<float>();
    q.d_occluded = d_occ.as<uint32_t>();
    q.stream     = nullptr; // with the blocking copies below, as render_to_host
    if (int rc = trace_rays_impl(s, &q, stats)) return rc;
    if (n == 0) return SP_OK;
    if (h_hits) SP_HIP(hipMemcpy(h_hits, d_hits.ptr, n * sizeof(sp_ray_hit), hipMemcpyDeviceToHost));
    if (h_normals) SP_HIP(hipMemcpy(h_normals, d_normals.ptr, n * 4 * sizeof(float), hipMemcpyDeviceToHost));
    if (h_occluded) SP_HIP(hipMemcpy(h_occluded, d_occ.ptr, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return SP_OK;
}

int sp_scene_trace_rays_host(sp_scene* s, int32_t mode, const sp_ray* h_rays, int64_t num_rays, sp_ray_hit* h_hits,
                             float* h_normals, uint32_t* h_occluded, sp_ray_query_stats* stats)
{
    if (!s) return fail(SP_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lock(s->mu); // residency is decided, and kept, under the scene's lock
    try {
        return trace_rays_host_impl(s, mode, h_rays, num_rays, h_hits, h_normals, h_occluded, stats);
    } catch (const std::exception& e) {
        return fail(SP_ERR_HIP, std::string("ray query failed: ") + e.what());
    }
}

// ---- feature buffers (SP_HAS_FEATURES; sp_features.hip) ------------------------------------------

// What the two calls share of their parameters: the tile list and the optional camera.
struct FeatureCommon {
    const int32_t*        tile_ids;
    const int32_t*        d_tile_ids;
    int64_t               num_tiles;
    const sp_camera_desc* camera;
};

// The shared refusals between "negative counts" and "no output pointer"; fills the tile list.  The
// tile count is the host scene's (the resident one's is equal), so the rules hold before any upload.
static int validate_feature_common(const sp_scene* s, const FeatureCommon& c, TileList& tiles)
{
    if (c.tile_ids && c.d_tile_ids) return fail(SP_ERR_ARG, "give tile_ids (host) or d_tile_ids (device), not both");
    sp_tile_count(s->host->image_width, s->host->image_height, &tiles.total);
    tiles.listed = c.tile_ids || c.d_tile_ids;
    tiles.n      = tiles.listed ? c.num_tiles : tiles.total;
    if (int rc = check_tile_list(tiles, c.tile_ids)) return rc;
    if (c.camera) {
        if (c.camera->film_width != s->host->image_width || c.camera->film_height != s->host->image_height)
            return fail(SP_ERR_ARG, "the camera's film size is not the scene's image size");
        if (!camera_finite(*c.camera)) return fail(SP_ERR_ARG, "the camera's transform is not finite");
    }
    return SP_OK;
}

static bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

static int check_feature_stats(const sp_feature_stats* stats)
{
    if (stats && stats->struct_size != sizeof(sp_feature_stats))
        return fail(SP_ERR_ARG, "sp_feature_stats.struct_size is not this library's");
    return SP_OK;
}

// Everything sp_scene_camera_rays refuses, in the header's order; changes nothing.  The scene's lock
// is held (s->device is read last).  device_pointers: the alignment rule of a device buffer.
static int validate_camera_rays(const sp_scene* s, const sp_camera_ray_params* p, const sp_ray* rays, const sp_feature_stats* stats,
                                bool device_pointers, TileList& tiles)
{
    if (p->struct_size != sizeof(sp_camera_ray_params)) return fail(SP_ERR_ARG, "sp_camera_ray_params.struct_size is not this library's");
    if (int rc = check_feature_stats(stats)) return rc;
    if (p->reserved0 != 0) return fail(SP_ERR_ARG, "sp_camera_ray_params.reserved must be 0");
    for (int32_t r : p->reserved)
        if (r != 0) return fail(SP_ERR_ARG, "sp_camera_ray_params.reserved must be 0");
    if (p->num_tiles < 0) return fail(SP_ERR_ARG, "num_tiles < 0");
    if ((uint64_t)p->first_sample + p->num_samples > ((uint64_t)1 << 32)) return fail(SP_ERR_ARG, "the sample range ends past 2^32");
    if (int rc = validate_feature_common(s, FeatureCommon{ p->tile_ids, p->d_tile_ids, p->num_tiles, p->camera }, tiles)) return rc;
    if (tiles.n > 0 && p->num_samples > 0 && !rays) return fail(SP_ERR_ARG, "no output pointer");
    if (device_pointers && misaligned(rays, 16)) return fail(SP_ERR_ARG, "d_rays must be 16-byte aligned");
    if (s->device < 0) return fail(SP_ERR_STATE, "sp_scene_upload must be called before sp_scene_camera_rays");
    return SP_OK;
}

// the resident scene with this call's camera (by value in the launch)
static spd::Scene feature_scene(const sp_scene* s, const sp_camera_desc* camera)
{
    spd::Scene sc = s->dev;
    if (camera) sc.camera = from_desc(camera->transform);
    return sc;
}

static void feature_stats_begin(const sp_scene* s, sp_feature_stats* stats)
{
    if (!stats) return;
    *stats             = sp_feature_stats{};
    stats->struct_size = sizeof(sp_feature_stats);
    stats->stack_depth = s->dev.stack_words;
}

static int camera_rays_impl(sp_scene* s, const sp_camera_ray_params* p, sp_ray* d_rays, sp_feature_stats* stats, bool device_pointers)
{
    TileList tiles;
    if (int rc = validate_camera_rays(s, p, d_rays, stats, device_pointers, tiles)) return rc;
    feature_stats_begin(s, stats);
    if (tiles.n == 0 || p->num_samples == 0) return SP_OK;
    const int64_t items = tiles.n * (int64_t)p->num_samples; // (tiles.n < 2^31: the ids are int32)
    if (items > (int64_t)INT32_MAX * 4) return fail(SP_ERR_UNSUPPORTED, "more (tile, sample) items than one launch takes");
    SP_HIP(hipSetDevice(s->device));
    RenderScratch&    r      = s->scratch;
    const hipStream_t stream = static_cast<hipStream_t>(p->stream);
    // the previous call on this scene (a render, a refit's successor, a query) comes first
    if (r.done_rec) SP_HIP(hipStreamWaitEvent(stream, r.ev_done, 0));
    spd::CameraRayArgs a{};
    a.tile_ids = p->d_tile_ids;
    if (p->tile_ids)
        if (int rc = stage_ids(s, p->tile_ids, tiles.n, stream, a.tile_ids)) return rc;
    a.num_tiles    = tiles.n;
    a.tiles_x      = (s->dev.width + 7) / 8;
    a.first_sample = p->first_sample;
    a.num_samples  = p->num_samples;
    a.rays         = d_rays;
    SP_HIP(hipEventRecord(r.ev0, stream));
    SP_HIP(spd::launch_camera_rays(feature_scene(s, p->camera), a, stream));
    if (int rc = end_call(s, stream)) return rc;
    if (!stats) return SP_OK; // stream order: only enqueued
    SP_HIP(hipEventSynchronize(r.ev1));
    SP_HIP(hipEventElapsedTime(&stats->kernel_ms, r.ev0, r.ev1));
    stats->launches    = 1;
    stats->camera_rays = (uint64_t)items * 64;
    return SP_OK;
}

int sp_scene_camera_rays(sp_scene* s, const sp_camera_ray_params* p, sp_ray* d_rays, sp_feature_stats* stats)
{
    if (!s || !p) return fail(SP_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lock(s->mu); // calls on one scene run one at a time (sp_scene::mu)
    try {
        return camera_rays_impl(s, p, d_rays, stats, true);
    } catch (const std::exception& e) {
        return fail(SP_ERR_HIP, std::string("sp_scene_camera_rays failed: ") + e.what());
    }
}

// the host form with the scene's lock held: the same refusals in the same order on the host array
// as given, then a device buffer of its own around the device form (trace_rays_host_impl's pattern)
static int camera_rays_host_impl(sp_scene* s, const sp_camera_ray_params* p, sp_ray* h_rays, sp_feature_stats* stats)
{
    TileList tiles;
    if (int rc = validate_camera_rays(s, p, h_rays, stats, false, tiles)) return rc;
    SP_HIP(hipSetDevice(s->device));
    const size_t  bytes = (size_t)tiles.n * p->num_samples * 64 * sizeof(sp_ray);
    DeviceScratch d_rays;
    if (bytes) SP_HIP(d_rays.reserve(bytes));
    sp_camera_ray_params dp = *p;
    dp.stream               = nullptr; // with the blocking copy below, as render_to_host
    if (int rc = camera_rays_impl(s, &dp, d_rays.as<sp_ray>(), stats, true)) return rc;
    if (bytes) SP_HIP(hipMemcpy(h_rays, d_rays.ptr, bytes, hipMemcpyDeviceToHost));
    return SP_OK;
}

int sp_scene_camera_rays_host(sp_scene* s, const sp_camera_ray_params* p, sp_ray* h_rays, sp_feature_stats* stats)
{
    if (!s || !p) return fail(SP_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lock(s->mu); // residency is decided, and kept, under the scene's lock
    try {
        return camera_rays_host_impl(s, p, h_rays, stats);
    } catch (const std::exception& e) {
        return fail(SP_ERR_HIP, std::string("sp_scene_camera_rays_host failed: ") + e.what());
    }
}

// Everything sp_scene_features refuses, in the header's order; changes nothing (validate_camera_rays)
static int validate_features(const sp_scene* s, const sp_feature_params* p, const sp_feature_stats* stats, bool device_pointers,
                             TileList& tiles)
{
    if (p->struct_size != sizeof(sp_feature_params)) return fail(SP_ERR_ARG, "sp_feature_params.struct_size is not this library's");
    if (int rc = check_feature_stats(stats)) return rc;
    for (int32_t r : p->reserved)
        if (r != 0) return fail(SP_ERR_ARG, "sp_feature_params.reserved must be 0");
    if (p->num_tiles < 0) return fail(SP_ERR_ARG, "num_tiles < 0");
    if (int rc = validate_feature_common(s, FeatureCommon{ p->tile_ids, p->d_tile_ids, p->num_tiles, p->camera }, tiles)) return rc;
    if (p->tile_samples && p->d_tile_samples) return fail(SP_ERR_ARG, "give tile_samples (host) or d_tile_samples (device), not both");
    if (!p->d_ids && !p->d_coverage && !p->d_depth && !p->d_normal && !p->d_albedo) return fail(SP_ERR_ARG, "no output pointer");
    if (device_pointers) {
        if (misaligned(p->d_ids, 16)) return fail(SP_ERR_ARG, "d_ids must be 16-byte aligned");
        if (misaligned(p->d_coverage, 4) || misaligned(p->d_depth, 4) || misaligned(p->d_normal, 4) || misaligned(p->d_albedo, 4) ||
            misaligned(p->d_tile_samples, 4) || misaligned(p->d_tile_ids, 4))
            return fail(SP_ERR_ARG, "d_coverage, d_depth, d_normal, d_albedo and the device lists must be 4-byte aligned");
    }
    if (s->device < 0) return fail(SP_ERR_STATE, "sp_scene_upload must be called before sp_scene_features");
    return SP_OK;
}

// after validate_features, with the scene's lock held
static int features_impl(sp_scene* s, const sp_feature_params* p, sp_feature_stats* stats, const TileList& tiles)
{
    feature_stats_begin(s, stats);
    if (tiles.n == 0) return SP_OK;
    const size_t lds_bytes = spd::feature_lds_bytes(s->dev);
    if (lds_bytes > 160 * 1024) return fail(SP_ERR_UNSUPPORTED, "BVH too deep for the LDS traversal stack");
    SP_HIP(hipSetDevice(s->device));
    RenderScratch&    r      = s->scratch;
    const hipStream_t stream = static_cast<hipStream_t>(p->stream);
    // the previous call on this scene (a render, a refit's successor, a query) comes first
    if (r.done_rec) SP_HIP(hipStreamWaitEvent(stream, r.ev_done, 0));
    spd::FeatureArgs a{};
    a.tile_ids     = p->d_tile_ids;
    a.tile_samples = p->d_tile_samples;
    // host lists go through one staging buffer of the ring: [tile ids][sample counts]
    if (p->tile_ids || p->tile_samples) {
        const size_t         n = (size_t)tiles.n;
        std::vector<int32_t> both;
        if (p->tile_ids) both.insert(both.end(), p->tile_ids, p->tile_ids + n);
        if (p->tile_samples) both.insert(both.end(), reinterpret_cast<const int32_t*>(p->tile_samples),
                                         reinterpret_cast<const int32_t*>(p->tile_samples) + n);
        const int32_t* d_both = nullptr;
        if (int rc = stage_ids(s, both.data(), (int64_t)both.size(), stream, d_both)) return rc;
        if (p->tile_ids) a.tile_ids = d_both;
        if (p->tile_samples) a.tile_samples = reinterpret_cast<const uint32_t*>(d_both + (p->tile_ids ? n : 0));
    }
    a.num_tiles = tiles.n;
    a.tiles_x   = (s->dev.width + 7) / 8;
    a.spp       = p->samples_per_pixel;
    a.ids       = reinterpret_cast<int4*>(p->d_ids);
    a.coverage  = p->d_coverage;
    a.depth     = p->d_depth;
    a.normal    = p->d_normal;
    a.albedo    = p->d_albedo;
    if (stats) { // counted only when asked for: words 5 and 6 of the render counters, which every call clears for itself
        a.counters = r.counters.as<unsigned long long>() + 5;
        SP_HIP(hipMemsetAsync(a.counters, 0, 2 * sizeof(unsigned long long), stream));
    }
    SP_HIP(hipEventRecord(r.ev0, stream));
    SP_HIP(spd::launch_features(feature_scene(s, p->camera), a, lds_bytes, stream));
    if (int rc = end_call(s, stream)) return rc;
    if (!stats) return SP_OK; // stream order: only enqueued
    SP_HIP(hipEventSynchronize(r.ev1));
    unsigned long long c[2] = { 0, 0 };
    SP_HIP(hipMemcpy(c, a.counters, sizeof(c), hipMemcpyDeviceToHost));
    SP_HIP(hipEventElapsedTime(&stats->kernel_ms, r.ev0, r.ev1));
    stats->launches    = 1;
    stats->camera_rays = c[0];
    stats->hits        = c[1];
    return SP_OK;
}

int sp_scene_features(sp_scene* s, const sp_feature_params* p, sp_feature_stats* stats)
{
    if (!s || !p) return fail(SP_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lock(s->mu); // calls on one scene run one at a time (sp_scene::mu)
    try {
        TileList tiles;
        if (int rc = validate_features(s, p, stats, true, tiles)) return rc;
        return features_impl(s, p, stats, tiles);
    } catch (const std::exception& e) {
        return fail(SP_ERR_HIP, std::string("sp_scene_features failed: ") + e.what());
    }
}

// the host form with the scene's lock held: the same refusals in the same order on the host arrays
// as given, then device buffers of its own around the device form (trace_rays_host_impl's pattern)
static int features_host_impl(sp_scene* s, const sp_feature_params* p, sp_feature_stats* stats)
{
    TileList tiles;
    if (int rc = validate_features(s, p, stats, false, tiles)) return rc;
    SP_HIP(hipSetDevice(s->device));
    const size_t      px = (size_t)tiles.n * 64;
    void* const       host[5]  = { p->d_ids, p->d_coverage, p->d_depth, p->d_normal, p->d_albedo };
    const size_t      bytes[5] = { px * 16, px * 4, px * 4, px * 12, px * 12 };
    DeviceScratch     dev[5];
    for (int k = 0; k < 5; ++k)
        if (host[k]) SP_HIP(dev[k].reserve(std::max<size_t>(bytes[k], 16)));
    sp_feature_params dp = *p;
    dp.d_ids      = dev[0].as<int32_t>();
    dp.d_coverage = dev[1].as<float>();
    dp.d_depth    = dev[2].as<float>();
    dp.d_normal   = dev[3].as<float>();
    dp.d_albedo   = dev[4].as<float>();
    dp.stream     = nullptr; // with the blocking copies below, as render_to_host
    if (int rc = features_impl(s, &dp, stats, tiles)) return rc;
    for (int k = 0; k < 5; ++k)
        if (host[k] && bytes[k]) SP_HIP(hipMemcpy(host[k], dev[k].ptr, bytes[k], hipMemcpyDeviceToHost));
    return SP_OK;
}

int sp_scene_features_host(sp_scene* s, const sp_feature_params* p, sp_feature_stats* stats)
{
    if (!s || !p) return fail(SP_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lock(s->mu); // residency is decided, and kept, under the scene's lock
    try {
        return features_host_impl(s, p, stats);
    } catch (const std::exception& e) {
        return fail(SP_ERR_HIP, std::string("sp_scene_features_host failed: ") + e.what());
    }
}

// ---- denoising (SP_HAS_DENOISE; sp_denoise.hip) ---------------------------------------------------

// A scene-free object: the frame, the tile list and the scratch the filter's launches share.  The
// device is first touched by the first run (prepare_denoiser), so creation validates without one.
struct sp_denoiser {
    std::mutex           mu;          // calls on one object run one at a time
    int32_t              device = 0, width = 0, height = 0, tiles_x = 0, tiles_y = 0;
    int64_t              n = 0;       // tile slots
    bool                 listed = false;
    std::vector<int32_t> host_ids;    // a host list's copy (the first run's upload reads it)
    const int32_t*       d_user_ids = nullptr; // a device list, read by the first run
    bool                 ready = false;
    DeviceScratch        ids, map, plane[2], guide, counters;
    Events<>             ev0, ev1, ev_done;
    bool                 done_rec = false;

    int64_t total() const { return (int64_t)tiles_x * tiles_y; }
    size_t  planned_bytes() const
    {
        if (n == 0) return 0;
        return (size_t)n * 64 * 16 * 3 + (listed ? (size_t)n * 4 : 0) + (size_t)total() * 4 + 2 * sizeof(unsigned long long);
    }
};

int sp_denoiser_create(const sp_denoiser_params* p, sp_denoiser** out)
{
    if (!p || !out) return fail(SP_ERR_ARG, "null argument");
    if (p->struct_size != sizeof(sp_denoiser_params)) return fail(SP_ERR_ARG, "sp_denoiser_params.struct_size is not this library's");
    for (int32_t r : p->reserved)
        if (r != 0) return fail(SP_ERR_ARG, "sp_denoiser_params.reserved must be 0");
    if (p->device < 0) return fail(SP_ERR_ARG, "device < 0");
    if (p->width < 1 || p->height < 1) return fail(SP_ERR_ARG, "width or height < 1");
    if (p->num_tiles < 0) return fail(SP_ERR_ARG, "num_tiles < 0");
    if (p->num_tiles > INT32_MAX) return fail(SP_ERR_ARG, "num_tiles above 2^31 - 1");
    const int64_t tiles_x = ((int64_t)p->width + 7) / 8, tiles_y = ((int64_t)p->height + 7) / 8;
    if (tiles_x * tiles_y > INT32_MAX) return fail(SP_ERR_ARG, "width x height: more tiles than an id can name");
    if (p->tile_ids && p->d_tile_ids) return fail(SP_ERR_ARG, "give tile_ids (host) or d_tile_ids (device), not both");
    TileList t;
    t.total  = tiles_x * tiles_y;
    t.listed = p->tile_ids || p->d_tile_ids;
    t.n      = t.listed ? p->num_tiles : t.total;
    if (int rc = check_tile_list(t, p->tile_ids)) return rc;
    if (p->tile_ids) {
        std::vector<bool> seen((size_t)t.total, false);
        for (int64_t i = 0; i < t.n; ++i) {
            if (seen[(size_t)p->tile_ids[i]]) return fail(SP_ERR_ARG, "tile_ids holds a repeated id");
            seen[(size_t)p->tile_ids[i]] = true;
        }
    }
    if (misaligned(p->d_tile_ids, 4)) return fail(SP_ERR_ARG, "d_tile_ids must be 4-byte aligned");
    try {
        sp_denoiser* d = new sp_denoiser;
        d->device      = p->device;
        d->width       = p->width;
        d->height      = p->height;
        d->tiles_x     = (int32_t)tiles_x;
        d->tiles_y     = (int32_t)tiles_y;
        d->n           = t.n;
        d->listed      = t.listed;
        d->d_user_ids  = p->d_tile_ids;
        if (p->tile_ids) d->host_ids.assign(p->tile_ids, p->tile_ids + t.n);
        *out = d;
        return SP_OK;
    } catch (const std::exception& e) {
        return fail(SP_ERR_HIP, std::string("sp_denoiser_create failed: ") + e.what());
    }
}

void sp_denoiser_free(sp_denoiser* d)
{
    if (!d) return;
    if (d->ready) {
        (void)hipSetDevice(d->device);
        if (d->done_rec) (void)hipEventSynchronize(d->ev_done); // queued work still uses the scratch
    }
    delete d;
}

int sp_denoiser_device_bytes(const sp_denoiser* d, int64_t* out)
{
    if (!d || !out) return fail(SP_ERR_ARG, "null argument");
    *out = (int64_t)d->planned_bytes();
    return SP_OK;
}

static bool sigma_ok(float s) { return std::isfinite(s) && s > 0.0f; }
static bool floor_ok(float f) { return std::isfinite(f) && f >= 0.0f; }

// [p, p + bytes) and [q, q + bytes_q) share a byte
static bool ranges_overlap(const void* p, size_t bytes, const void* q, size_t bytes_q)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return p && q && a < b + bytes_q && b < a + bytes;
}

// Everything sp_denoiser_run refuses, in the header's order; changes nothing
static int validate_denoise(const sp_denoiser* d, const sp_denoise_params* p, const sp_denoise_stats* stats, bool device_pointers)
{
    if (p->struct_size != sizeof(sp_denoise_params)) return fail(SP_ERR_ARG, "sp_denoise_params.struct_size is not this library's");
    if (stats && stats->struct_size != sizeof(sp_denoise_stats)) return fail(SP_ERR_ARG, "sp_denoise_stats.struct_size is not this library's");
    if (p->reserved0 != 0) return fail(SP_ERR_ARG, "sp_denoise_params.reserved must be 0");
    for (int32_t r : p->reserved)
        if (r != 0) return fail(SP_ERR_ARG, "sp_denoise_params.reserved must be 0");
    if (p->flags & ~SP_DENOISE_DEMODULATE) return fail(SP_ERR_ARG, "sp_denoise_params.flags: unknown flag");
    if (p->iterations < 1 || p->iterations > SP_DENOISE_MAX_ITERATIONS) return fail(SP_ERR_ARG, "iterations must be 1 .. 8");
    if (!sigma_ok(p->sigma_color)) return fail(SP_ERR_ARG, "sigma_color must be finite and > 0");
    if (p->d_normal && !sigma_ok(p->sigma_normal)) return fail(SP_ERR_ARG, "sigma_normal must be finite and > 0");
    if (p->d_depth && !sigma_ok(p->sigma_depth)) return fail(SP_ERR_ARG, "sigma_depth must be finite and > 0");
    if (p->d_coverage && !sigma_ok(p->sigma_coverage)) return fail(SP_ERR_ARG, "sigma_coverage must be finite and > 0");
    if (!floor_ok(p->albedo_floor)) return fail(SP_ERR_ARG, "albedo_floor must be finite and >= 0");
    if (!floor_ok(p->depth_floor)) return fail(SP_ERR_ARG, "depth_floor must be finite and >= 0");
    if (d->n > 0 && !p->d_color) return fail(SP_ERR_ARG, "d_color is missing");
    if (d->n > 0 && !p->d_out) return fail(SP_ERR_ARG, "d_out is missing");
    if ((p->flags & SP_DENOISE_DEMODULATE) && (!p->d_albedo || !p->d_coverage))
        return fail(SP_ERR_ARG, "SP_DENOISE_DEMODULATE needs d_albedo and d_coverage");
    if (device_pointers && (misaligned(p->d_color, 4) || misaligned(p->d_albedo, 4) || misaligned(p->d_normal, 4) ||
                            misaligned(p->d_depth, 4) || misaligned(p->d_coverage, 4) || misaligned(p->d_out, 4)))
        return fail(SP_ERR_ARG, "d_color, d_albedo, d_normal, d_depth, d_coverage and d_out must be 4-byte aligned");
    const size_t px = (size_t)d->n * 64 * sizeof(float);
    if (p->d_out != p->d_color && ranges_overlap(p->d_out, px * 3, p->d_color, px * 3))
        return fail(SP_ERR_ARG, "d_out overlaps d_color without being equal to it");
    if (ranges_overlap(p->d_out, px * 3, p->d_albedo, px * 3) || ranges_overlap(p->d_out, px * 3, p->d_normal, px * 3) ||
        ranges_overlap(p->d_out, px * 3, p->d_depth, px) || ranges_overlap(p->d_out, px * 3, p->d_coverage, px))
        return fail(SP_ERR_ARG, "d_out overlaps d_albedo, d_normal, d_depth or d_coverage");
    return SP_OK;
}

// The first run's share: the object's memory, its copy of the list and the inverse map, on `stream`
static int prepare_denoiser(sp_denoiser* d, hipStream_t stream, int& launches)
{
    if (d->ready) return SP_OK;
    const size_t slots = (size_t)d->n * 64;
    for (DeviceScratch& pl : d->plane) SP_HIP(pl.reserve(slots * 16));
    SP_HIP(d->guide.reserve(slots * 16));
    SP_HIP(d->map.reserve((size_t)d->total() * 4));
    SP_HIP(d->counters.reserve(2 * sizeof(unsigned long long)));
    for (hipEvent_t* e : { &d->ev0[0], &d->ev1[0], &d->ev_done[0] })
        if (!*e) SP_HIP(hipEventCreate(e));
    if (d->listed) {
        SP_HIP(d->ids.reserve((size_t)d->n * 4));
        if (!d->host_ids.empty()) { // (the object keeps the vector: the source outlives the copy, no host wait)
            SP_HIP(hipMemcpyAsync(d->ids.ptr, d->host_ids.data(), (size_t)d->n * 4, hipMemcpyHostToDevice, stream));
        } else {
            SP_HIP(hipMemcpyAsync(d->ids.ptr, d->d_user_ids, (size_t)d->n * 4, hipMemcpyDeviceToDevice, stream));
        }
    }
    SP_HIP(hipMemsetAsync(d->map.ptr, 0xff, (size_t)d->total() * 4, stream)); // -1: absent
    SP_HIP(spd::launch_denoise_map(d->ids.as<int32_t>(), d->n, (int32_t)d->total(), d->map.as<int32_t>(), stream));
    ++launches;
    d->ready = true;
    return SP_OK;
}

// after validate_denoise, with the object's lock held
static int denoise_impl(sp_denoiser* d, const sp_denoise_params* p, sp_denoise_stats* stats)
{
    if (stats) {
        *stats             = sp_denoise_stats{};
        stats->struct_size = sizeof(sp_denoise_stats);
    }
    if (d->n == 0) return SP_OK;
    SP_HIP(hipSetDevice(d->device));
    const hipStream_t stream = static_cast<hipStream_t>(p->stream);
    // the object's previous run comes first: it uses the same scratch
    if (d->done_rec) SP_HIP(hipStreamWaitEvent(stream, d->ev_done, 0));
    int launches = 0;
    if (int rc = prepare_denoiser(d, stream, launches)) return rc;
    spd::DenoiseArgs a{};
    a.tile_ids     = d->listed ? d->ids.as<int32_t>() : nullptr;
    a.slot_of_tile = d->map.as<int32_t>();
    a.num_tiles    = d->n;
    a.tiles_x      = d->tiles_x;
    a.tiles_y      = d->tiles_y;
    a.width        = d->width;
    a.height       = d->height;
    a.color        = p->d_color;
    a.albedo       = p->d_albedo;
    a.normal       = p->d_normal;
    a.depth        = p->d_depth;
    a.coverage     = p->d_coverage;
    a.out          = p->d_out;
    a.plane[0]     = d->plane[0].as<float4>();
    a.plane[1]     = d->plane[1].as<float4>();
    a.guide        = d->guide.as<float4>();
    a.sigma_depth  = p->sigma_depth;
    a.depth_floor  = p->depth_floor == 0.0f ? spdn::k_depth_floor : p->depth_floor;
    a.albedo_floor = p->albedo_floor == 0.0f ? spdn::k_albedo_floor : p->albedo_floor;
    a.demodulate   = (p->flags & SP_DENOISE_DEMODULATE) ? 1 : 0;
    if (stats) { // counted only when asked for
        a.counters = d->counters.as<unsigned long long>();
        SP_HIP(hipMemsetAsync(a.counters, 0, 2 * sizeof(unsigned long long), stream));
    }
    SP_HIP(hipEventRecord(d->ev0, stream));
    SP_HIP(spd::launch_denoise_prepare(a, stream));
    for (int i = 0; i < p->iterations; ++i) {
        const spdn::Level L = spdn::level_constants(i, p->sigma_color, p->sigma_normal, p->sigma_coverage, p->d_normal != nullptr,
                                                    p->d_coverage != nullptr);
        SP_HIP(spd::launch_denoise_level(a, L, i, p->iterations, stream));
    }
    launches += 1 + p->iterations;
    SP_HIP(hipEventRecord(d->ev1, stream));
    SP_HIP(hipEventRecord(d->ev_done, stream));
    d->done_rec = true;
    if (!stats) return SP_OK; // stream order: only enqueued
    SP_HIP(hipEventSynchronize(d->ev1));
    unsigned long long c[2] = { 0, 0 };
    SP_HIP(hipMemcpy(c, a.counters, sizeof(c), hipMemcpyDeviceToHost));
    SP_HIP(hipEventElapsedTime(&stats->kernel_ms, d->ev0, d->ev1));
    stats->launches = launches;
    stats->pixels   = c[0];
    stats->taps     = c[1];
    return SP_OK;
}

int sp_denoiser_run(sp_denoiser* d, const sp_denoise_params* p, sp_denoise_stats* stats)
{
    if (!d || !p) return fail(SP_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lock(d->mu);
    try {
        if (int rc = validate_denoise(d, p, stats, true)) return rc;
        return denoise_impl(d, p, stats);
    } catch (const std::exception& e) {
        return fail(SP_ERR_HIP, std::string("sp_denoiser_run failed: ") + e.what());
    }
}

// the host form with the object's lock held: the same refusals in the same order on the host arrays
// as given, then device buffers of its own around the device form (features_host_impl's pattern)
static int denoise_host_impl(sp_denoiser* d, const sp_denoise_params* p, sp_denoise_stats* stats)
{
    if (int rc = validate_denoise(d, p, stats, false)) return rc;
    if (d->n == 0) return denoise_impl(d, p, stats);
    SP_HIP(hipSetDevice(d->device));
    const size_t      px       = (size_t)d->n * 64 * sizeof(float);
    const float*      host[5]  = { p->d_color, p->d_albedo, p->d_normal, p->d_depth, p->d_coverage };
    const size_t      bytes[5] = { px * 3, px * 3, px * 3, px, px };
    DeviceScratch     dev[5];
    for (int k = 0; k < 5; ++k)
        if (host[k]) {
            SP_HIP(dev[k].reserve(bytes[k]));
            SP_HIP(hipMemcpy(dev[k].ptr, host[k], bytes[k], hipMemcpyHostToDevice));
        }
    sp_denoise_params dp = *p;
    dp.d_color    = dev[0].as<float>();
    dp.d_albedo   = dev[1].as<float>();
    dp.d_normal   = dev[2].as<float>();
    dp.d_depth    = dev[3].as<float>();
    dp.d_coverage = dev[4].as<float>();
    dp.d_out      = dev[0].as<float>(); // in place: d_out may equal d_color
    dp.stream     = nullptr;            // with the blocking copies around it, as render_to_host
    if (int rc = denoise_impl(d, &dp, stats)) return rc;
    SP_HIP(hipMemcpy(p->d_out, dev[0].ptr, bytes[0], hipMemcpyDeviceToHost));
    return SP_OK;
}

int sp_denoiser_run_host(sp_denoiser* d, const sp_denoise_params* p, sp_denoise_stats* stats)
{
    if (!d || !p) return fail(SP_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lock(d->mu);
    try {
        return denoise_host_impl(d, p, stats);
    } catch (const std::exception& e) {
        return fail(SP_ERR_HIP, std::string("sp_denoiser_run_host failed: ") + e.what());
    }
}

int sp_scene_device_bytes(const sp_scene* s, int64_t* bytes)
{
    if (!s || !bytes || s->device < 0) return fail(SP_ERR_STATE, "scene not uploaded");
    *bytes = (int64_t)s->device_bytes();
    return SP_OK;
}

int sp_scene_bvh_info(const sp_scene* s, int32_t* depth, int64_t* nodes, int64_t* slots)
{
    if (!s || s->device < 0) return fail(SP_ERR_STATE, "scene not uploaded");
    if (depth) *depth = s->sizes.geom_depth;
    if (nodes) *nodes = (int64_t)s->sizes.geom_nodes;
    if (slots) *slots = (int64_t)s->sizes.geom_slots;
    return SP_OK;
}

} // extern "C"
