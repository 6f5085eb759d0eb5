// sp_devbuild.hip -- the parts of sp_devbuild.hpp that are code of their own: the scan, and the
// opening and ending of a binary build.
#include "sp_devbuild.hpp"

#include <rocprim/device/device_scan.hpp>

namespace spb {

hipError_t Scan::reserve(Arena& mem, size_t max_n)
{
    const hipError_t e = rocprim::exclusive_scan(nullptr, bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, max_n,
                                                 rocprim::plus<uint32_t>(), hipStream_t(0));
    return e != hipSuccess ? e : mem.get(&tmp, bytes);
}

hipError_t Scan::run(uint32_t* in, uint32_t* out, size_t n) const
{
    size_t need = bytes; // (the query was for the largest size)
    return rocprim::exclusive_scan(tmp, need, in, out, 0u, n, rocprim::plus<uint32_t>(), hipStream_t(0));
}

void open_binary(size_t n, int max_leaf, const char* what, sph::Bvh& out, DeviceTree* keep)
{
    if (keep) keep->reset();
    out = sph::Bvh{};
    if (n >= (size_t(1) << sph::BVH_AXIS_SHIFT)) throw sph::SpError(SP_ERR_UNSUPPORTED, std::string("too many primitives for the ") + what);
    if (max_leaf < 1 || max_leaf > 4) throw sph::SpError(SP_ERR_ARG, std::string(what) + ": leaf size must be 1..4");
}

int finish_binary(Stage& stage, Node* d_nodes, uint32_t m, uint32_t* d_order, uint32_t n, DeviceTree* keep, sph::Bvh& out,
                  double& ms_copy_back)
{
    if (keep) {
        stage.mem.release(d_nodes);
        stage.mem.release(d_order);
        keep->nodes   = d_nodes;
        keep->order   = d_order;
        keep->n_nodes = m;
        keep->n_slots = n;
        return SP_OK;
    }
    out.nodes.resize(m);
    out.prim_order.resize(n);
    SPB_HIP(hipMemcpy(out.nodes.data(), d_nodes, (size_t)m * sizeof(Node), hipMemcpyDeviceToHost));
    static_assert(sizeof(int32_t) == sizeof(uint32_t), "prim_order");
    SPB_HIP(hipMemcpy(out.prim_order.data(), d_order, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    stage.lap(ms_copy_back);
    return SP_OK;
}

} // namespace spb
