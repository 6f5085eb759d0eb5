// sp_build.hip -- linear BVH build on the device.
//
// Stages, each its own launch: centroid bounds (two-stage reduction, no float atomics), Morton
// codes, a stable radix sort of (code, id) pairs (rocprim, the only library call), the Karras
// ranges with one thread per internal node, an exclusive count of the kept candidates, node
// emission with the leaf boxes, and the internal boxes in passes.  No launch reads bytes that
// another workgroup wrote in that same launch, except the pass words of the box fit, where a
// stale or same-pass value only delays a node by one pass (sp_devbuild.hpp launch_fit_pass).  No
// kernel spins.
#include "sp_devbuild.hpp"
#include "../common/sp_lbvh.h"

#include <rocprim/device/device_radix_sort.hpp>

namespace spb {
namespace {

constexpr uint32_t MAX_PARTIAL = 1024; // blocks of the first reduction stage
constexpr int      MAX_PASSES  = 160;  // tree height <= 64 + 32 key bits; beyond it the build fails

// min / max of six values per thread over the block; thread 0 holds the result
__device__ void block_bounds(float v[6])
{
    __shared__ float s[6][BLOCK];
    const int        t = (int)threadIdx.x;
    for (int k = 0; k < 6; ++k) s[k][t] = v[k];
    __syncthreads();
    for (int w = BLOCK / 2; w > 0; w >>= 1) {
        if (t < w)
            for (int k = 0; k < 3; ++k) {
                s[k][t]     = lbvh::lower(s[k][t], s[k][t + w]);
                s[k + 3][t] = lbvh::upper(s[k + 3][t], s[k + 3][t + w]);
            }
        __syncthreads();
    }
    for (int k = 0; k < 6; ++k) v[k] = s[k][0];
}

__global__ __launch_bounds__(BLOCK) void lb_centroid_bounds(const sph::PrimBounds* __restrict__ bounds, uint32_t n,
                                                            float* __restrict__ partial)
{
    float v[6] = { INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY };
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BLOCK)
        for (int d = 0; d < 3; ++d) {
            const float c = spm::centre(bounds[i].lo[d], bounds[i].hi[d]);
            v[d]          = lbvh::lower(v[d], c);
            v[d + 3]      = lbvh::upper(v[d + 3], c);
        }
    block_bounds(v);
    if (threadIdx.x == 0)
        for (int k = 0; k < 6; ++k) partial[(size_t)blockIdx.x * 6 + k] = v[k];
}

// one block: partial[0 .. count) -> cb[6]
__global__ __launch_bounds__(BLOCK) void lb_centroid_bounds_final(const float* __restrict__ partial, uint32_t count,
                                                                  float* __restrict__ cb)
{
    float v[6] = { INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY };
    for (uint32_t i = threadIdx.x; i < count; i += BLOCK)
        for (int d = 0; d < 3; ++d) {
            v[d]     = lbvh::lower(v[d], partial[(size_t)i * 6 + d]);
            v[d + 3] = lbvh::upper(v[d + 3], partial[(size_t)i * 6 + d + 3]);
        }
    block_bounds(v);
    if (threadIdx.x == 0)
        for (int k = 0; k < 6; ++k) cb[k] = v[k];
}

__global__ __launch_bounds__(BLOCK) void lb_codes(const sph::PrimBounds* __restrict__ bounds, uint32_t n,
                                                  const float* __restrict__ cb, uint64_t* __restrict__ codes,
                                                  uint32_t* __restrict__ ids)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    uint32_t q[3];
    for (int d = 0; d < 3; ++d) q[d] = lbvh::cell(spm::centre(bounds[i].lo[d], bounds[i].hi[d]), cb[d], cb[d + 3]);
    codes[i] = lbvh::code(q[0], q[1], q[2]);
    ids[i]   = i;
}

// One thread per internal node i of n - 1: its range and split, and the keep flag of its two
// children: kept when this node covers more than max_leaf positions, which then holds for every
// ancestor too.  Each candidate has one parent, so each flag has one writer; thread 0 also sets
// the root's.
__global__ __launch_bounds__(BLOCK) void lb_hierarchy(const uint64_t* __restrict__ codes, uint32_t n, uint32_t max_leaf,
                                                      lbvh::Range* __restrict__ rng, uint32_t* __restrict__ keep)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n - 1u) return;
    const lbvh::Range r = lbvh::node_range(codes, (int64_t)n, (int64_t)i);
    rng[i]              = r;
    const uint32_t kept = (r.last - r.first + 1u > max_leaf) ? 1u : 0u;
    keep[lbvh::left_cand(r, n)]  = kept;
    keep[lbvh::right_cand(r, n)] = kept;
    if (i == 0) keep[0] = 1u;
}

// One thread per candidate c of 2n - 1: a kept candidate writes its node at index[c]; a leaf also
// gets its box (its primitives' bounds folded in slot order) and pass word 1.
__global__ __launch_bounds__(BLOCK) void lb_emit(const sph::PrimBounds* __restrict__ bounds, const uint32_t* __restrict__ order,
                                                 const lbvh::Range* __restrict__ rng, const uint32_t* __restrict__ keep,
                                                 const uint32_t* __restrict__ index, uint32_t n, uint32_t max_leaf,
                                                 uint32_t m, Node* __restrict__ nodes, uint32_t* __restrict__ pass_of)
{
    const uint32_t c = blockIdx.x * BLOCK + threadIdx.x;
    if (c >= 2u * n - 1u || !keep[c]) return;
    const uint32_t k = index[c];
    if (k >= m) return; // (cannot happen: m is the count of kept candidates)
    Node nd;
    if (c < n - 1u && rng[c].last - rng[c].first + 1u > max_leaf) {
        const lbvh::Range r = rng[c];
        for (int d = 0; d < 3; ++d) { nd.lo[d] = 0.0f; nd.hi[d] = 0.0f; }
        nd.a       = index[lbvh::left_cand(r, n)] | r.axis << sph::BVH_AXIS_SHIFT;
        nd.b       = index[lbvh::right_cand(r, n)];
        nodes[k]   = nd;
        pass_of[k] = 0u;
        return;
    }
    const uint32_t first = c < n - 1u ? rng[c].first : c - (n - 1u);
    const uint32_t count = c < n - 1u ? rng[c].last - rng[c].first + 1u : 1u;
    for (int d = 0; d < 3; ++d) { nd.lo[d] = INFINITY; nd.hi[d] = -INFINITY; }
    for (uint32_t s = 0; s < count; ++s) {
        const sph::PrimBounds b = bounds[order[first + s]];
        for (int d = 0; d < 3; ++d) {
            nd.lo[d] = spm::sse_min(nd.lo[d], b.lo[d]);
            nd.hi[d] = spm::sse_max(nd.hi[d], b.hi[d]);
        }
    }
    nd.a       = first;
    nd.b       = count | sph::BVH_LEAF;
    nodes[k]   = nd;
    pass_of[k] = 1u;
}

} // namespace

int build_lbvh_device(const std::vector<sph::PrimBounds>& bounds, int max_leaf, sph::Bvh& out, BuildStats& st, std::string& err,
                      bool timed, DeviceTree* keep)
{
    st             = BuildStats{};
    const size_t n = bounds.size();
    open_binary(n, max_leaf, "linear BVH", out, keep);
    if (n <= 1) { // nothing to sort or link: empty, or one leaf
        out = sph::build_bvh_lbvh(bounds, max_leaf);
        return SP_OK;
    }
    Stage  stage("device BVH build", err, timed);
    Arena& mem = stage.mem; // (the name the error texts carry)

    const uint32_t un = (uint32_t)n, total = 2u * un - 1u;
    sph::PrimBounds* d_bounds = nullptr;
    float *          d_partial = nullptr, *d_cb = nullptr;
    uint64_t *       d_code_in = nullptr, *d_code = nullptr;
    uint32_t *       d_id_in = nullptr, *d_order = nullptr;
    SPB_HIP(mem.get(&d_bounds, n));
    SPB_HIP(mem.get(&d_partial, (size_t)MAX_PARTIAL * 6));
    SPB_HIP(mem.get(&d_cb, 6));
    SPB_HIP(mem.get(&d_code_in, n));
    SPB_HIP(mem.get(&d_code, n));
    SPB_HIP(mem.get(&d_id_in, n));
    SPB_HIP(mem.get(&d_order, n));
    SPB_HIP(hipMemcpy(d_bounds, bounds.data(), n * sizeof(sph::PrimBounds), hipMemcpyHostToDevice));
    stage.lap(st.ms_bounds_up);

    // ---- centroid bounds, codes
    const uint32_t nb1 = std::min(MAX_PARTIAL, blocks_for(n));
    hipLaunchKernelGGL(lb_centroid_bounds, dim3(nb1), dim3(BLOCK), 0, 0, d_bounds, un, d_partial);
    hipLaunchKernelGGL(lb_centroid_bounds_final, dim3(1), dim3(BLOCK), 0, 0, d_partial, nb1, d_cb);
    hipLaunchKernelGGL(lb_codes, dim3(blocks_for(n)), dim3(BLOCK), 0, 0, d_bounds, un, d_cb, d_code_in, d_id_in);
    SPB_HIP(hipGetLastError());
    stage.lap(st.ms_codes);

    // ---- stable sort of (code, id) by code
    {
        size_t tmp_bytes = 0;
        SPB_HIP(rocprim::radix_sort_pairs(nullptr, tmp_bytes, d_code_in, d_code, d_id_in, d_order, n, 0u, 63u, hipStream_t(0)));
        unsigned char* d_tmp = nullptr;
        SPB_HIP(mem.get(&d_tmp, tmp_bytes));
        SPB_HIP(rocprim::radix_sort_pairs(d_tmp, tmp_bytes, d_code_in, d_code, d_id_in, d_order, n, 0u, 63u, hipStream_t(0)));
    }
    stage.lap(st.ms_sort);

    // ---- ranges, kept candidates, numbering
    lbvh::Range* d_rng = nullptr;
    uint32_t *   d_keep = nullptr, *d_index = nullptr;
    SPB_HIP(mem.get(&d_rng, n - 1));
    SPB_HIP(mem.get(&d_keep, total));
    SPB_HIP(mem.get(&d_index, total));
    hipLaunchKernelGGL(lb_hierarchy, dim3(blocks_for(n - 1)), dim3(BLOCK), 0, 0, d_code, un, (uint32_t)max_leaf, d_rng, d_keep);
    SPB_HIP(hipGetLastError());
    Scan scan;
    SPB_HIP(scan.reserve(mem, total));
    SPB_HIP(scan.run(d_keep, d_index, total));
    uint32_t last_index = 0, last_keep = 0;
    SPB_HIP(hipMemcpy(&last_index, d_index + (total - 1), 4, hipMemcpyDeviceToHost));
    SPB_HIP(hipMemcpy(&last_keep, d_keep + (total - 1), 4, hipMemcpyDeviceToHost));
    const uint32_t m = last_index + last_keep;
    if (m == 0 || m > total) return stage.refuse("the kept-node count is out of range");

    // ---- nodes and leaf boxes, then the internal boxes in passes
    Node*     d_nodes = nullptr;
    uint32_t *d_pass = nullptr, *d_fitted = nullptr;
    SPB_HIP(mem.get(&d_nodes, m));
    SPB_HIP(mem.get(&d_pass, m));
    SPB_HIP(mem.get(&d_fitted, MAX_PASSES + 1));
    SPB_HIP(hipMemset(d_fitted, 0, (MAX_PASSES + 1) * sizeof(uint32_t)));
    hipLaunchKernelGGL(lb_emit, dim3(blocks_for(total)), dim3(BLOCK), 0, 0, d_bounds, d_order, d_rng, d_keep, d_index, un,
                       (uint32_t)max_leaf, m, d_nodes, d_pass);
    SPB_HIP(hipGetLastError());
    stage.lap(st.ms_hierarchy);
    // a binary tree with m nodes has (m - 1) / 2 internal ones
    const uint32_t internal = (m - 1u) / 2u;
    uint32_t       done     = 0;
    for (uint32_t pass = 2; done < internal; ++pass) {
        if (pass > (uint32_t)MAX_PASSES) return stage.refuse("the box fit did not finish");
        launch_fit_pass(d_nodes, m, d_pass, pass, d_fitted + pass);
        SPB_HIP(hipGetLastError());
        uint32_t now = 0;
        SPB_HIP(hipMemcpy(&now, d_fitted + pass, 4, hipMemcpyDeviceToHost));
        ++st.passes;
        if (now == 0) return stage.refuse("a fit pass made no progress");
        done += now;
    }
    stage.lap(st.ms_fit);
    st.peak_bytes = mem.peak;
    if (const int rc = finish_binary(stage, d_nodes, m, d_order, un, keep, out, st.ms_copy_back)) return rc;
    out.max_depth = keep ? st.passes + 1 : sph::bvh_walk_depth(out.nodes);
    return SP_OK;
}

} // namespace spb
