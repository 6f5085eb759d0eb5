// sp_finish.hip -- the device finish: 8-wide collapse, primitive records and
// parent links from a binary BVH resident in device memory, the bytes of the host path.
//
// The collapse runs level by level (sph::build_wide_levels is the host restatement).  A wide node is
// an item; the items of a level sit side by side in arrays of `cap` entries, level after level.  Per
// level: collapse every item (one thread each, spw::collapse), count its inner children, exclusive
// scan (rocprim), scatter the children's binary roots behind the level.  Then subtree sums bottom-up,
// bases top-down, and every record at its final index.  Every hand-off between workgroups is a
// kernel boundary; no kernel spins or waits on a counter, and nothing is placed with atomics (the
// error word alone is an atomicMax of the error code).
#include "sp_finish.hpp"
#include "sp_devbuild.hpp"
#include "../common/sp_wide.h"

namespace spf {
namespace {

using spb::BLOCK;
using spb::blocks_for;
using spb::Node;

// per item, in arrays of `cap` entries
struct Items {
    uint32_t* root;       // binary root
    uint32_t* info;       // imask | span << 8 | own << 16 | lmask << 24
    uint32_t* kid;        // 8 per item: binary node in slot s
    uint32_t* words;      // 20 per item: the record without its bases
    uint32_t* count;      // inner children
    uint32_t* first;      // exclusive scan of count within the level
    uint32_t *n_sub, *l_sub;
    uint32_t *record, *child_base, *leaf_base;
};

__device__ inline uint32_t info_imask(uint32_t i) { return i & 0xffu; }
__device__ inline uint32_t info_span(uint32_t i) { return (i >> 8) & 0xffu; }
__device__ inline uint32_t info_own(uint32_t i) { return (i >> 16) & 0xffu; }
__device__ inline uint32_t info_lmask(uint32_t i) { return i >> 24; }

// one thread per item of the level [off, off + cnt)
__global__ __launch_bounds__(BLOCK) void fw_collapse(const Node* __restrict__ nodes, uint32_t n_nodes, Items it, uint32_t off,
                                                     uint32_t cnt, uint32_t* __restrict__ err)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= cnt) return;
    const uint32_t  v = off + i;
    spw::Collapsed c;
    const int       e = spw::collapse(nodes, n_nodes, it.root[v], c);
    if (e != spw::OK) {
        atomicMax(err, (uint32_t)e);
        it.info[v]  = 0u;
        it.count[v] = 0u;
        for (int k = 0; k < 8; ++k) it.kid[(size_t)v * 8 + k] = 0u;
        for (int k = 0; k < 20; ++k) it.words[(size_t)v * 20 + k] = 0u;
        return;
    }
    it.info[v]  = c.imask | (uint32_t)c.span << 8 | c.own << 16 | c.lmask << 24;
    it.count[v] = (uint32_t)__popc(c.imask);
    for (int k = 0; k < 8; ++k) it.kid[(size_t)v * 8 + k] = c.kid[k];
    for (int k = 0; k < 20; ++k) it.words[(size_t)v * 20 + k] = c.w[k];
}

// the inner children of item v become items off + cnt + first[v] ... in slot order; the last item
// also writes the next level's size
__global__ __launch_bounds__(BLOCK) void fw_scatter(Items it, uint32_t off, uint32_t cnt, uint32_t cap,
                                                    uint32_t* __restrict__ next_count, uint32_t* __restrict__ err)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= cnt) return;
    const uint32_t v     = off + i;
    const uint32_t imask = info_imask(it.info[v]);
    uint64_t       k     = (uint64_t)off + cnt + it.first[v];
    for (int s = 0; s < 8; ++s) {
        if (!((imask >> s) & 1u)) continue;
        if (k < cap) it.root[k] = it.kid[(size_t)v * 8 + s];
        else atomicMax(err, (uint32_t)spw::ERR_LINKS);
        ++k;
    }
    if (i == cnt - 1u) *next_count = it.first[v] + (uint32_t)__popc(imask);
}

// N = span + sum N(child), L = own + sum L(child); the children's sums come from an earlier launch
__global__ __launch_bounds__(BLOCK) void fw_sums(Items it, uint32_t off, uint32_t cnt, uint32_t cap, uint32_t* __restrict__ err)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= cnt) return;
    const uint32_t v    = off + i;
    const uint32_t info = it.info[v];
    uint64_t       n = info_span(info), l = info_own(info);
    uint64_t       k = (uint64_t)off + cnt + it.first[v];
    for (int s = 0; s < 8; ++s) {
        if (!((info_imask(info) >> s) & 1u)) continue;
        if (k < cap) { n += it.n_sub[k]; l += it.l_sub[k]; }
        ++k;
    }
    if (n + 1u >= spw::MAX_RECORDS) {
        atomicMax(err, (uint32_t)spw::ERR_RECORDS);
        n = 0;
    }
    it.n_sub[v] = (uint32_t)n;
    it.l_sub[v] = (uint32_t)l;
}

// top-down: an item hands its children their record index and bases (its own came from an earlier
// launch; item 0 is the root and sets its own)
__global__ __launch_bounds__(BLOCK) void fw_bases(Items it, uint32_t off, uint32_t cnt, uint32_t cap)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= cnt) return;
    const uint32_t v = off + i;
    uint32_t       my_cb, my_lb;
    if (v == 0u) {
        it.record[0]     = 0u;
        it.child_base[0] = my_cb = 1u;
        it.leaf_base[0]  = my_lb = 0u;
    } else {
        my_cb = it.child_base[v];
        my_lb = it.leaf_base[v];
    }
    const uint32_t info = it.info[v];
    uint32_t       cb = my_cb + info_span(info), lb = my_lb + info_own(info);
    uint64_t       k = (uint64_t)off + cnt + it.first[v];
    for (int s = 0; s < 8; ++s) {
        if (!((info_imask(info) >> s) & 1u)) continue;
        if (k < cap) {
            it.record[k]     = my_cb + (uint32_t)s;
            it.child_base[k] = cb;
            it.leaf_base[k]  = lb;
            cb += it.n_sub[k];
            lb += it.l_sub[k];
        }
        ++k;
    }
}

// one thread per item of all levels: the record at its final index, the slots from leaf_base
__global__ __launch_bounds__(BLOCK) void fw_emit(const Node* __restrict__ nodes, Items it, uint32_t total, uint32_t records,
                                                 uint32_t wide_slots, uint32_t* __restrict__ wnodes, uint32_t* __restrict__ slot_of)
{
    const uint32_t v = blockIdx.x * BLOCK + threadIdx.x;
    if (v >= total) return;
    const uint32_t rec = it.record[v];
    if (rec >= records) return; // (cannot happen: the bases follow from the sums)
    for (int k = 0; k < 20; ++k) {
        uint32_t w = it.words[(size_t)v * 20 + k];
        if (k == 4) w = it.child_base[v];
        if (k == 5) w = it.leaf_base[v];
        wnodes[(size_t)rec * 20 + k] = w;
    }
    const uint32_t lmask = info_lmask(it.info[v]);
    uint64_t       at    = it.leaf_base[v];
    for (int s = 0; s < 8; ++s) {
        if (!((lmask >> s) & 1u)) continue;
        const Node     lf    = nodes[it.kid[(size_t)v * 8 + s]];
        const uint32_t count = lf.b & ~spw::LEAF;
        for (uint32_t j = 0; j < count; ++j, ++at)
            if (at < wide_slots) slot_of[at] = lf.a + j;
    }
}

// slot_tri, slot_code: the record (spb::packed_record) and the code of the primitive in each slot,
// by prim_order
__global__ __launch_bounds__(BLOCK) void fw_pack(const uint32_t* __restrict__ order, uint32_t n_slots,
                                                 const uint32_t* __restrict__ codes, uint32_t n_prims,
                                                 const float* __restrict__ verts, uint64_t n_verts,
                                                 const uint32_t* __restrict__ indices, uint64_t n_indices,
                                                 float4* __restrict__ slot_tri, uint32_t* __restrict__ slot_code)
{
    const uint32_t sl = blockIdx.x * BLOCK + threadIdx.x;
    if (sl >= n_slots) return;
    const uint32_t p    = order[sl];
    const uint32_t code = p < n_prims ? codes[p] : 0u;
    float4         v[3];
    spb::packed_record(code, verts, n_verts, indices, n_indices, v);
    slot_code[sl] = code;
    for (int k = 0; k < 3; ++k) slot_tri[3ull * sl + k] = v[k];
}

// wslot_tri: the records in the wide tree's slot order (slot_tri is from an earlier launch)
__global__ __launch_bounds__(BLOCK) void fw_pack_wide(const uint32_t* __restrict__ slot_of, uint32_t wide_slots, uint32_t n_slots,
                                                      const float4* __restrict__ slot_tri, float4* __restrict__ wslot_tri)
{
    const uint32_t ws = blockIdx.x * BLOCK + threadIdx.x;
    if (ws >= wide_slots) return;
    const uint32_t b = slot_of[ws];
    for (int k = 0; k < 3; ++k)
        wslot_tri[3ull * ws + k] = b < n_slots ? slot_tri[3ull * b + k] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// one thread per node: an internal node is the parent of its two children (sp_capi.hip parent_links;
// the array starts as zeros, so the root is its own parent)
__global__ __launch_bounds__(BLOCK) void fw_parents(const Node* __restrict__ nodes, uint32_t n_nodes, uint32_t* __restrict__ parents)
{
    const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
    if (k >= n_nodes || (nodes[k].b & spw::LEAF)) return;
    const uint32_t l = nodes[k].a & spw::CHILD_MASK, r = nodes[k].b;
    if (l < n_nodes) parents[l] = k;
    if (r < n_nodes) parents[r] = k;
}

// the caller's outputs while they are filled: emptied again unless the finish ends well
struct Outputs {
    FinishOut& o;
    bool       keep = false;
    ~Outputs()
    {
        if (!keep) o.reset();
    }
};

} // namespace

int finish_device(const FinishIn& in, FinishOut& out, FinishStats& st, std::string& err, bool timed)
{
    out.reset();
    st = FinishStats{};
    spb::Stage  stage("device finish", err, timed);
    spb::Arena& mem = stage.mem; // (the name the error texts carry)
    Outputs     res{ out };
    auto        refuse = [&](int code) { return stage.refuse(spw::error_text(code)); };
    auto alloc_out = [&](void** p, size_t& bytes_out, size_t bytes) -> hipError_t {
        const hipError_t e = hipMalloc(p, bytes);
        if (e == hipSuccess) bytes_out = bytes;
        else *p = nullptr;
        return e;
    };
    if (in.n_nodes == 0 || in.n_slots == 0) return SP_OK; // no bounded primitive: no tree, no records
    const Node* nodes = in.d_nodes;

    // ---- inputs that are not resident: the order (host builder), codes, vertex positions
    const uint32_t* d_order = in.d_order;
    if (!d_order) {
        uint32_t* p = nullptr;
        SPB_HIP(mem.get(&p, in.n_slots));
        static_assert(sizeof(int32_t) == sizeof(uint32_t), "prim_order");
        SPB_HIP(hipMemcpy(p, in.h_order, (size_t)in.n_slots * 4, hipMemcpyHostToDevice));
        d_order = p;
    }
    uint32_t* d_codes = nullptr;
    float*    d_verts = nullptr;
    SPB_HIP(mem.get(&d_codes, in.n_prims));
    SPB_HIP(mem.get(&d_verts, in.n_verts * 3));
    if (in.n_prims) SPB_HIP(hipMemcpy(d_codes, in.h_codes, (size_t)in.n_prims * 4, hipMemcpyHostToDevice));
    static_assert(sizeof(spm::f3) == 12, "vertex layout");
    if (in.n_verts) SPB_HIP(hipMemcpy(d_verts, in.h_verts, in.n_verts * 12, hipMemcpyHostToDevice));
    stage.lap(st.ms_inputs_up);

    // ---- records in the binary tree's order
    SPB_HIP(alloc_out(&res.o.slot_tri, res.o.slot_tri_bytes, (size_t)in.n_slots * 3 * sizeof(float4)));
    SPB_HIP(alloc_out(&res.o.slot_code, res.o.slot_code_bytes, (size_t)in.n_slots * sizeof(uint32_t)));
    hipLaunchKernelGGL(fw_pack, dim3(blocks_for(in.n_slots)), dim3(BLOCK), 0, 0, d_order, in.n_slots, d_codes, in.n_prims, d_verts,
                       (uint64_t)in.n_verts, in.d_indices, (uint64_t)in.n_indices, static_cast<float4*>(res.o.slot_tri),
                       static_cast<uint32_t*>(res.o.slot_code));
    SPB_HIP(hipGetLastError());
    stage.lap(st.ms_pack);

    // ---- parent links
    if (in.want_parents) {
        SPB_HIP(alloc_out(&res.o.parents, res.o.parents_bytes, (size_t)in.n_nodes * sizeof(uint32_t)));
        SPB_HIP(hipMemset(res.o.parents, 0, res.o.parents_bytes));
        hipLaunchKernelGGL(fw_parents, dim3(blocks_for(in.n_nodes)), dim3(BLOCK), 0, 0, nodes, in.n_nodes,
                           static_cast<uint32_t*>(res.o.parents));
        SPB_HIP(hipGetLastError());
        stage.lap(st.ms_parents);
    }

    if (in.want_wide) {
        // every wide node swallows at least one internal binary node; a lone leaf makes one
        const uint32_t cap = std::max(1u, (in.n_nodes - 1u) / 2u);
        Items          it{};
        uint32_t *     d_err = nullptr, *d_next = nullptr;
        SPB_HIP(mem.get(&it.root, cap));
        SPB_HIP(mem.get(&it.info, cap));
        SPB_HIP(mem.get(&it.kid, (size_t)cap * 8));
        SPB_HIP(mem.get(&it.words, (size_t)cap * 20));
        SPB_HIP(mem.get(&it.count, cap));
        SPB_HIP(mem.get(&it.first, cap));
        SPB_HIP(mem.get(&it.n_sub, cap));
        SPB_HIP(mem.get(&it.l_sub, cap));
        SPB_HIP(mem.get(&it.record, cap));
        SPB_HIP(mem.get(&it.child_base, cap));
        SPB_HIP(mem.get(&it.leaf_base, cap));
        SPB_HIP(mem.get(&d_err, 1));
        SPB_HIP(mem.get(&d_next, 1));
        SPB_HIP(hipMemset(d_err, 0, 4));
        SPB_HIP(hipMemset(it.root, 0, 4)); // item 0: the binary root
        spb::Scan scan;
        SPB_HIP(scan.reserve(mem, cap));

        // 1. top-down: one launch set per level; the host reads the next level's size
        std::vector<uint32_t> level_off{ 0u }, level_cnt{ 1u };
        for (;;) {
            const uint32_t off = level_off.back(), cnt = level_cnt.back();
            hipLaunchKernelGGL(fw_collapse, dim3(blocks_for(cnt)), dim3(BLOCK), 0, 0, nodes, in.n_nodes, it, off, cnt, d_err);
            SPB_HIP(hipGetLastError());
            SPB_HIP(scan.run(it.count + off, it.first + off, cnt));
            hipLaunchKernelGGL(fw_scatter, dim3(blocks_for(cnt)), dim3(BLOCK), 0, 0, it, off, cnt, cap, d_next, d_err);
            SPB_HIP(hipGetLastError());
            uint32_t next = 0;
            SPB_HIP(hipMemcpy(&next, d_next, 4, hipMemcpyDeviceToHost));
            if (next == 0) break;
            if ((uint64_t)off + cnt + next > cap) return refuse(spw::ERR_LINKS);
            if (level_off.size() >= (size_t)spw::MAX_LEVELS) return refuse(spw::ERR_LEVELS);
            level_off.push_back(off + cnt);
            level_cnt.push_back(next);
        }
        const uint32_t total = level_off.back() + level_cnt.back();
        st.levels            = (int)level_off.size();
        stage.lap(st.ms_collapse);
        // 2. bottom-up: subtree sums
        for (size_t l = level_off.size(); l-- > 0;) {
            hipLaunchKernelGGL(fw_sums, dim3(blocks_for(level_cnt[l])), dim3(BLOCK), 0, 0, it, level_off[l], level_cnt[l], cap, d_err);
            SPB_HIP(hipGetLastError());
        }
        stage.lap(st.ms_sums);
        // 3. top-down: bases
        for (size_t l = 0; l < level_off.size(); ++l) {
            hipLaunchKernelGGL(fw_bases, dim3(blocks_for(level_cnt[l])), dim3(BLOCK), 0, 0, it, level_off[l], level_cnt[l], cap);
            SPB_HIP(hipGetLastError());
        }
        // the error word, once; with it the root's sums
        uint32_t code = 0, n_root = 0, l_root = 0;
        SPB_HIP(hipMemcpy(&code, d_err, 4, hipMemcpyDeviceToHost));
        SPB_HIP(hipMemcpy(&n_root, it.n_sub, 4, hipMemcpyDeviceToHost));
        SPB_HIP(hipMemcpy(&l_root, it.l_sub, 4, hipMemcpyDeviceToHost));
        stage.lap(st.ms_bases);
        if (code != 0) return refuse((int)code);
        if (l_root != in.n_slots) return refuse(spw::ERR_EMPTY_LEVEL); // the levels ended with primitives left over
        const uint32_t records = 1u + n_root;
        // 4. records and slots at their final places; holes stay zero
        uint32_t* d_slot_of = nullptr;
        SPB_HIP(mem.get(&d_slot_of, l_root));
        SPB_HIP(hipMemset(d_slot_of, 0xff, (size_t)l_root * 4));
        SPB_HIP(alloc_out(&res.o.wnodes, res.o.wnodes_bytes, (size_t)records * 80));
        SPB_HIP(hipMemset(res.o.wnodes, 0, res.o.wnodes_bytes));
        hipLaunchKernelGGL(fw_emit, dim3(blocks_for(total)), dim3(BLOCK), 0, 0, nodes, it, total, records, l_root,
                           static_cast<uint32_t*>(res.o.wnodes), d_slot_of);
        SPB_HIP(hipGetLastError());
        stage.lap(st.ms_emit);
        SPB_HIP(alloc_out(&res.o.wslot_tri, res.o.wslot_tri_bytes, (size_t)l_root * 3 * sizeof(float4)));
        hipLaunchKernelGGL(fw_pack_wide, dim3(blocks_for(l_root)), dim3(BLOCK), 0, 0, d_slot_of, l_root, in.n_slots,
                           static_cast<const float4*>(res.o.slot_tri), static_cast<float4*>(res.o.wslot_tri));
        SPB_HIP(hipGetLastError());
        res.o.records    = records;
        res.o.wide_slots = l_root;
        res.o.depth      = (int)level_off.size();
    }
    SPB_HIP(hipDeviceSynchronize()); // the scratch goes away with this call
    stage.lap(st.ms_pack);
    st.peak_bytes = mem.peak;
    res.keep      = true;
    return SP_OK;
}

} // namespace spf
