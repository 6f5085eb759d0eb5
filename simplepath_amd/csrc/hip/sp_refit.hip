// sp_refit.hip -- the device refit: a resident scene follows new vertex positions
// without a new tree.
//
// Stages, each its own launch: the records of the binary tree's slots and of the wide tree's slots
// from the new positions (the code of a slot names its primitive: slot_code, and p0.w of a wide
// record); the leaves' boxes and, in passes, the internal boxes of the binary tree (the linear
// build's pass, spb::launch_fit_pass); the records of the 8-wide tree bottom-up in passes of the same kind, each record quantised
// again from the exact boxes of its slots (sp_refit.h).  Every hand-off between workgroups is a
// kernel boundary: a node or record is fitted in pass k only from children whose pass word, written
// by an earlier launch, lies in [1, k).  No kernel spins or counts arrivals, nothing is placed with
// an atomic; the two fitted counts and the error word are the only atomics, and the host reads
// them once, after the last pass.  The number of passes is the height of each tree, which the
// resident scene knows.
#include "sp_refit.hpp"
#include "sp_devbuild.hpp"
#include "../common/sp_refit.h"

namespace spr {
namespace {

using spb::BLOCK;
using spb::blocks_for;
using spb::Node;
using spb::packed_record;
using spm::CODE_MASK;
using spm::CODE_SHIFT;
using spm::KIND_TRIANGLE;
static_assert(sizeof(sph::PrimBounds) == 24, "bounds layout");

// one thread per slot of the binary tree's order
__global__ __launch_bounds__(BLOCK) void rf_pack(const uint32_t* __restrict__ slot_code, uint32_t n_slots,
                                                 const float* __restrict__ verts, uint64_t n_verts,
                                                 const uint32_t* __restrict__ indices, uint64_t n_indices,
                                                 float4* __restrict__ slot_tri)
{
    const uint32_t sl = blockIdx.x * BLOCK + threadIdx.x;
    if (sl >= n_slots) return;
    float4 v[3];
    packed_record(slot_code[sl], verts, n_verts, indices, n_indices, v);
    for (int k = 0; k < 3; ++k) slot_tri[3ull * sl + k] = v[k];
}

// one thread per slot of the wide tree's order: its code is in its own p0.w
__global__ __launch_bounds__(BLOCK) void rf_pack_wide(uint32_t wide_slots, const float* __restrict__ verts, uint64_t n_verts,
                                                      const uint32_t* __restrict__ indices, uint64_t n_indices,
                                                      float4* wslot_tri)
{
    const uint32_t ws = blockIdx.x * BLOCK + threadIdx.x;
    if (ws >= wide_slots) return;
    const float4 p0 = wslot_tri[3ull * ws];
    float4       v[3];
    packed_record(__float_as_uint(p0.w), verts, n_verts, indices, n_indices, v);
    for (int k = 0; k < 3; ++k) wslot_tri[3ull * ws + k] = v[k];
}

// bounds of the primitive in a freshly packed record: a triangle's from its positions, another
// bounded primitive's from the table by shape index
__device__ inline Box record_box(const float4* __restrict__ rec, const sph::PrimBounds* __restrict__ shapes, uint32_t n_shapes)
{
    const float4   p0 = rec[0], p1 = rec[1], p2 = rec[2];
    const uint32_t code = __float_as_uint(p0.w), kind = code >> CODE_SHIFT, idx = code & CODE_MASK;
    if (kind == KIND_TRIANGLE) {
        const float a[3] = { p0.x, p0.y, p0.z }, b[3] = { p1.x, p1.y, p1.z }, c[3] = { p2.x, p2.y, p2.z };
        return tri_box(a, b, c);
    }
    Box r = empty_box();
    if (idx < n_shapes)
        for (int d = 0; d < 3; ++d) { r.lo[d] = shapes[idx].lo[d]; r.hi[d] = shapes[idx].hi[d]; }
    return r;
}

// One thread per binary node: a leaf folds its slots' bounds in slot order and gets pass word 1, an
// internal node pass word 0.
__global__ __launch_bounds__(BLOCK) void rf_leaf_boxes(Node* __restrict__ nodes, uint32_t m, const float4* __restrict__ slot_tri,
                                                       uint32_t n_slots, const sph::PrimBounds* __restrict__ shapes,
                                                       uint32_t n_shapes, uint32_t* __restrict__ pass_of)
{
    const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
    if (k >= m) return;
    const uint32_t a = nodes[k].a, b = nodes[k].b;
    if (!(b & spw::LEAF)) {
        pass_of[k] = 0u;
        return;
    }
    const uint32_t count = b & ~spw::LEAF;
    Box            box   = empty_box();
    for (uint32_t s = 0; s < count; ++s) {
        const uint64_t sl = (uint64_t)a + s;
        if (sl >= n_slots) break;
        fold(box, record_box(slot_tri + 3ull * sl, shapes, n_shapes));
    }
    for (int d = 0; d < 3; ++d) { nodes[k].lo[d] = box.lo[d]; nodes[k].hi[d] = box.hi[d]; }
    pass_of[k] = 1u;
}

// what the two wide kernels share
struct WideArgs {
    uint4*                 wnodes; // 5 per record
    uint32_t               records;
    const float4*          wslot_tri;
    uint32_t               wide_slots;
    const sph::PrimBounds* shapes;
    uint32_t               n_shapes;
    float*                 exact; // 6 per record: the union of everything beneath it
    uint32_t*              pass_of;
    uint32_t*              err;
};

__device__ inline void load_record(const WideArgs& g, uint32_t r, uint32_t w[20])
{
    for (int q = 0; q < 5; ++q) {
        const uint4 x = g.wnodes[5ull * r + q];
        w[4 * q] = x.x; w[4 * q + 1] = x.y; w[4 * q + 2] = x.z; w[4 * q + 3] = x.w;
    }
}

// Fits record r from `w`, its words as they stand: leaf slots from the wide slots' records, inner
// slots from the children's exact boxes (the caller has seen their pass words).  Writes the words
// that change, the exact box, and the pass word.
__device__ inline void fit_record(const WideArgs& g, uint32_t r, uint32_t w[20], uint32_t pass)
{
    const uint32_t imask = rec_imask(w), occupied = rec_occupied(w);
    Box            slot[8];
    for (int s = 0; s < 8; ++s) {
        slot[s] = empty_box();
        if ((imask >> s) & 1u) {
            const uint64_t c = (uint64_t)w[4] + (uint32_t)s;
            if (c < g.records)
                for (int d = 0; d < 3; ++d) { slot[s].lo[d] = g.exact[6 * c + d]; slot[s].hi[d] = g.exact[6 * c + 3 + d]; }
            continue;
        }
        const uint32_t meta = rec_meta(w, s), cnt = meta >> 5, off = meta & 31u;
        for (uint32_t j = 0; j < cnt; ++j) {
            const uint64_t ws = (uint64_t)w[5] + off + j;
            if (ws >= g.wide_slots) break;
            fold(slot[s], record_box(g.wslot_tri + 3ull * ws, g.shapes, g.n_shapes));
        }
    }
    Box       u;
    const int e = refit_record(w, slot, occupied, u);
    if (e != spw::OK) atomicMax(g.err, (uint32_t)e);
    else if (occupied) {
        g.wnodes[5ull * r]     = make_uint4(w[0], w[1], w[2], w[3]);
        g.wnodes[5ull * r + 2] = make_uint4(w[8], w[9], w[10], w[11]);
        g.wnodes[5ull * r + 3] = make_uint4(w[12], w[13], w[14], w[15]);
        g.wnodes[5ull * r + 4] = make_uint4(w[16], w[17], w[18], w[19]);
    }
    for (int d = 0; d < 3; ++d) { g.exact[6ull * r + d] = u.lo[d]; g.exact[6ull * r + 3 + d] = u.hi[d]; }
    g.pass_of[r] = pass;
}

// One thread per record: one without inner children (a hole among them, which stays zero) is
// fitted here, as pass 1; the others get pass word 0.
__global__ __launch_bounds__(BLOCK) void rf_wide_leaf_slots(WideArgs g, uint32_t* __restrict__ fitted)
{
    const uint32_t r   = blockIdx.x * BLOCK + threadIdx.x;
    int            did = 0;
    if (r < g.records) {
        uint32_t w[20];
        load_record(g, r, w);
        if (rec_imask(w) != 0u) g.pass_of[r] = 0u;
        else {
            fit_record(g, r, w, 1u);
            did = 1;
        }
    }
    const int total = __syncthreads_count(did);
    if (threadIdx.x == 0 && total) atomicAdd(fitted, (uint32_t)total);
}

// Pass `pass` >= 2: a record whose every inner child carries a pass word in [1, pass) -- written,
// with that child's exact box, by an earlier launch -- is fitted.  Nothing else reads the words it
// writes during the refit.
__global__ __launch_bounds__(BLOCK) void rf_wide_pass(WideArgs g, uint32_t pass, uint32_t* __restrict__ fitted)
{
    const uint32_t r   = blockIdx.x * BLOCK + threadIdx.x;
    int            did = 0;
    if (r < g.records && g.pass_of[r] == 0u) {
        uint32_t w[20];
        load_record(g, r, w);
        const uint32_t imask = rec_imask(w);
        bool           ready = true;
        for (int s = 0; s < 8; ++s) {
            if (!((imask >> s) & 1u)) continue;
            const uint64_t c = (uint64_t)w[4] + (uint32_t)s;
            if (c >= g.records) { ready = false; continue; }
            const uint32_t pc = g.pass_of[c];
            ready             = ready && pc >= 1u && pc < pass;
        }
        if (ready) {
            fit_record(g, r, w, pass);
            did = 1;
        }
    }
    const int total = __syncthreads_count(did);
    if (threadIdx.x == 0 && total) atomicAdd(fitted, (uint32_t)total);
}

} // namespace

int refit_device(const RefitIn& in, RefitStats& st, std::string& err, bool timed)
{
    st               = RefitStats{};
    const auto  start = spb::Stage::clock::now();
    spb::Stage  stage("device refit", err, timed);
    spb::Arena& mem = stage.mem; // (the name the error texts carry)

    // ---- scratch: the new positions, the shape bounds, pass words, exact boxes, three counters
    const bool             wide = in.d_wnodes != nullptr && in.records != 0;
    float*                 d_verts = nullptr;
    sph::PrimBounds*       d_shapes = nullptr;
    uint32_t *             d_pass = nullptr, *d_wpass = nullptr, *d_ctr = nullptr; // ctr: binary fitted, wide fitted, error
    float*                 d_exact = nullptr;
    SPB_HIP(mem.get(&d_verts, in.n_verts * 3));
    SPB_HIP(mem.get(&d_shapes, in.n_shapes));
    SPB_HIP(mem.get(&d_pass, in.n_nodes));
    SPB_HIP(mem.get(&d_ctr, 4));
    if (wide) {
        SPB_HIP(mem.get(&d_wpass, in.records));
        SPB_HIP(mem.get(&d_exact, (size_t)in.records * 6));
    }
    SPB_HIP(hipMemset(d_ctr, 0, 16));
    static_assert(sizeof(spm::f3) == 12, "vertex layout");
    if (in.n_verts) SPB_HIP(hipMemcpy(d_verts, in.h_verts, in.n_verts * 12, hipMemcpyHostToDevice));
    if (in.n_shapes) SPB_HIP(hipMemcpy(d_shapes, in.h_shape_bounds, (size_t)in.n_shapes * sizeof(sph::PrimBounds), hipMemcpyHostToDevice));
    if (in.h_normals && in.d_normals && in.n_verts) SPB_HIP(hipMemcpy(in.d_normals, in.h_normals, in.n_verts * 12, hipMemcpyHostToDevice));
    stage.lap(st.ms_copy);

    if (in.n_nodes != 0 && in.n_slots != 0) {
        // ---- records
        hipLaunchKernelGGL(rf_pack, dim3(blocks_for(in.n_slots)), dim3(BLOCK), 0, 0, in.d_slot_code, in.n_slots, d_verts,
                           (uint64_t)in.n_verts, in.d_indices, (uint64_t)in.n_indices, in.d_slot_tri);
        if (wide && in.wide_slots)
            hipLaunchKernelGGL(rf_pack_wide, dim3(blocks_for(in.wide_slots)), dim3(BLOCK), 0, 0, in.wide_slots, d_verts,
                               (uint64_t)in.n_verts, in.d_indices, (uint64_t)in.n_indices, in.d_wslot_tri);
        SPB_HIP(hipGetLastError());
        stage.lap(st.ms_pack);

        // ---- the binary tree: leaves, then one pass per level above them
        Node* nodes = in.d_nodes;
        hipLaunchKernelGGL(rf_leaf_boxes, dim3(blocks_for(in.n_nodes)), dim3(BLOCK), 0, 0, nodes, in.n_nodes, in.d_slot_tri, in.n_slots,
                           d_shapes, in.n_shapes, d_pass);
        for (int pass = 2; pass <= in.geom_depth; ++pass) {
            spb::launch_fit_pass(nodes, in.n_nodes, d_pass, (uint32_t)pass, d_ctr);
            ++st.binary_passes;
        }
        SPB_HIP(hipGetLastError());
        stage.lap(st.ms_binary);

        // ---- the 8-wide tree
        if (wide) {
            const WideArgs g{ reinterpret_cast<uint4*>(in.d_wnodes), in.records, in.d_wslot_tri, in.wide_slots, d_shapes, in.n_shapes,
                              d_exact,                               d_wpass,    d_ctr + 2 };
            hipLaunchKernelGGL(rf_wide_leaf_slots, dim3(blocks_for(in.records)), dim3(BLOCK), 0, 0, g, d_ctr + 1);
            for (int pass = 2; pass <= in.wide_depth; ++pass) {
                hipLaunchKernelGGL(rf_wide_pass, dim3(blocks_for(in.records)), dim3(BLOCK), 0, 0, g, (uint32_t)pass, d_ctr + 1);
                ++st.wide_passes;
            }
            SPB_HIP(hipGetLastError());
        }
    }
    // the totals and the error word, once; the scratch goes away with this call
    uint32_t ctr[4] = {};
    SPB_HIP(hipMemcpy(ctr, d_ctr, 16, hipMemcpyDeviceToHost)); // (waits for the null stream)
    SPB_HIP(hipDeviceSynchronize());
    stage.lap(st.ms_wide);
    st.peak_bytes = mem.peak;
    st.ms_total   = std::chrono::duration<double, std::milli>(spb::Stage::clock::now() - start).count();
    if (ctr[2] != 0) return stage.refuse(spw::error_text((int)ctr[2]));
    if (in.n_nodes != 0 && in.n_slots != 0) {
        if (ctr[0] != (in.n_nodes - 1u) / 2u) return stage.refuse("the box fit did not reach every internal node");
        if (wide && ctr[1] != in.records) return stage.refuse("the wide fit did not reach every record");
    }
    return SP_OK;
}

} // namespace spr
