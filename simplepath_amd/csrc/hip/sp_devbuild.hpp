// sp_devbuild.hpp -- what the device stages of the accelerator build share:
// sp_build.hip, sp_sah_build.hip, sp_finish.hip and sp_refit.hip.  The scratch arena, the per-call
// context with its timer and error report, the scan, the box-fit pass, a slot's record, and the
// opening and ending of a binary build.  Everything runs on the null stream.
#pragma once

#include "sp_build.hpp"
#include "../common/sp_box.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <utility>
#include <vector>

namespace spb {

using Node = sph::BvhNode;
static_assert(spm::KIND_TRIANGLE == (uint32_t)SP_PRIM_TRIANGLE, "a triangle's code");

constexpr int BLOCK = 256;
inline uint32_t blocks_for(uint64_t threads, uint32_t block = BLOCK) { return (uint32_t)((threads + block - 1) / block); }

// a stage's device scratch: freed when the stage returns, whichever way.  `bytes` is what is alive
// now (a released block stays counted: the stage made it), `peak` the most that ever was.
class Arena {
    std::vector<std::pair<void*, size_t>> blocks;
    size_t                                bytes = 0;

public:
    size_t peak = 0;
    ~Arena()
    {
        for (const auto& b : blocks) (void)hipFree(b.first);
    }
    template <typename T>
    hipError_t get(T** out, size_t count)
    {
        void*            p = nullptr;
        const size_t     b = std::max<size_t>(count * sizeof(T), 16);
        const hipError_t e = hipMalloc(&p, b);
        if (e != hipSuccess) return e;
        blocks.emplace_back(p, b);
        bytes += b;
        peak = std::max(peak, bytes);
        *out = static_cast<T*>(p);
        return hipSuccess;
    }
    // hands a block over to the caller, who frees it
    void release(void* p)
    {
        blocks.erase(std::remove_if(blocks.begin(), blocks.end(), [p](const auto& b) { return b.first == p; }), blocks.end());
    }
    // frees a block now
    void drop(void* p)
    {
        for (const auto& b : blocks)
            if (b.first == p) bytes -= b.second;
        release(p);
        (void)hipFree(p);
    }
};

// One call of a stage: its scratch, and how it reports.  `lap` adds the time since the last lap to
// `ms` after waiting for the device; an untimed call takes no times at all (nothing reads them).
// `fail` and `refuse` set `err` to "<stage>: ..." and return the code, for `return stage.fail(..)`.
struct Stage {
    using clock = std::chrono::steady_clock;
    const char*       name;
    std::string&      err;
    const bool        timed;
    Arena             mem;
    clock::time_point t0 = clock::now();

    Stage(const char* name_, std::string& err_, bool timed_) : name(name_), err(err_), timed(timed_) {}
    void lap(double& ms)
    {
        if (!timed) return;
        (void)hipDeviceSynchronize();
        const auto t1 = clock::now();
        ms += std::chrono::duration<double, std::milli>(t1 - t0).count();
        t0 = t1;
    }
    int refuse(const char* why, int code = SP_ERR_HIP)
    {
        err = std::string(name) + ": " + why;
        return code;
    }
    int fail(const char* what, hipError_t e) // a HIP call's error, which it clears
    {
        err = std::string(name) + ": " + what + ": " + hipGetErrorString(e);
        (void)hipGetLastError();
        return SP_ERR_HIP;
    }
};
// in a function that returns a status and whose Stage is called `stage`
#define SPB_HIP(call)                                            \
    do {                                                         \
        const hipError_t e__ = (call);                           \
        if (e__ != hipSuccess) return stage.fail(#call, e__);    \
    } while (0)

// exclusive plus-scan of uint32_t (rocprim), its temporary taken once for the largest n
struct Scan {
    unsigned char* tmp   = nullptr;
    size_t         bytes = 0;
    hipError_t reserve(Arena& mem, size_t max_n);
    hipError_t run(uint32_t* in, uint32_t* out, size_t n) const;
};

// Box fit, pass `pass` >= 2, one thread per node of m: an internal node (pass word 0) whose
// children both carry a pass word in [1, pass) merges their boxes, takes `pass` as its word, and is
// counted in *fitted.  Such a word was written by an earlier launch, and so was the box it
// announces.  A word another workgroup writes in this launch reads as 0 or as `pass`; either
// leaves the node to a later pass, where it belongs: its height is above `pass` then.  Grid and
// block are the launcher's; the caller's loop decides how many passes run and when it reads.
// The kernel has internal linkage: each user launches the copy in its own code object, so a refit
// in a process that built nothing on the device loads no other stage's kernels.
namespace {
__global__ __launch_bounds__(BLOCK) void fit_pass(Node* __restrict__ nodes, uint32_t m, uint32_t* __restrict__ pass_of, uint32_t pass,
                                                  uint32_t* __restrict__ fitted)
{
    const uint32_t k   = blockIdx.x * BLOCK + threadIdx.x;
    int            did = 0;
    if (k < m && pass_of[k] == 0u) {
        const uint32_t l = nodes[k].a & sph::BVH_CHILD_MASK, r = nodes[k].b;
        if (l < m && r < m) {
            const uint32_t pl = pass_of[l], pr = pass_of[r];
            if (pl >= 1u && pl < pass && pr >= 1u && pr < pass) {
                for (int d = 0; d < 3; ++d) {
                    nodes[k].lo[d] = spm::sse_min(nodes[l].lo[d], nodes[r].lo[d]);
                    nodes[k].hi[d] = spm::sse_max(nodes[l].hi[d], nodes[r].hi[d]);
                }
                pass_of[k] = pass;
                did        = 1;
            }
        }
    }
    const int total = __syncthreads_count(did);
    if (threadIdx.x == 0 && total) atomicAdd(fitted, (uint32_t)total);
}

void launch_fit_pass(Node* nodes, uint32_t m, uint32_t* pass_of, uint32_t pass, uint32_t* fitted)
{
    hipLaunchKernelGGL(fit_pass, dim3(blocks_for(m)), dim3(BLOCK), 0, 0, nodes, m, pass_of, pass, fitted);
}
} // namespace

// The opening of a binary build over n primitives: empties `out` and `keep`, and throws what the
// host builders throw.  `what` names the tree in both texts.
void open_binary(size_t n, int max_leaf, const char* what, sph::Bvh& out, DeviceTree* keep);
// Its ending: `keep` takes the two blocks out of the stage's arena, or they are copied back into
// `out` and the copy is lapped into `ms_copy_back`.
int finish_binary(Stage& stage, Node* d_nodes, uint32_t m, uint32_t* d_order, uint32_t n, DeviceTree* keep, sph::Bvh& out,
                  double& ms_copy_back);

// The record of a slot: the three positions of the primitive named by `code`, zero for what is not
// a triangle or does not lie in the arrays, and the code in p0.w.
__device__ inline void packed_record(uint32_t code, const float* __restrict__ verts, uint64_t n_verts,
                                     const uint32_t* __restrict__ indices, uint64_t n_indices, float4 v[3])
{
    const uint32_t kind = code >> spm::CODE_SHIFT, idx = code & spm::CODE_MASK;
    for (int k = 0; k < 3; ++k) v[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (kind == spm::KIND_TRIANGLE && 3ull * idx + 2ull < n_indices)
        for (int k = 0; k < 3; ++k) {
            const uint64_t vi = indices[3ull * idx + k];
            if (vi < n_verts) v[k] = make_float4(verts[3 * vi], verts[3 * vi + 1], verts[3 * vi + 2], 0.0f);
        }
    v[0].w = __uint_as_float(code);
}

} // namespace spb
