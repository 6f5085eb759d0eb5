// sp_adaptive.hip -- the small kernels of a round on an adaptive progress object (sp_adaptive_round,
// DESIGN.md §14): tile errors and the selection, the stable compaction of the selected slots into
// the render kernel's queue (sp_adapt_kernel, sp_mega.hpp), and the resolve of the tiles the round
// does not render.  One wave per tile where a tile is the unit; nothing here meets another wave's
// address, so there is no atomic.
#include "sp_launch.hpp"

namespace spd {
namespace {
constexpr int TILES_PER_BLOCK = 4;    // one wave each
constexpr int COMPACT_THREADS = 1024; // one block: 16 waves scan 1024 queue positions per step

__device__ __forceinline__ uint32_t compact_bits(uint32_t a) // every second bit of a byte
{
    a = a & 0x55u;
    a = (a | (a >> 1)) & 0x33u;
    a = (a | (a >> 2)) & 0x0fu;
    return a;
}

// Per-pixel error after n samples: the standard error of the mean luminance over the mean (floored).
// Division and sqrt are correctly rounded (the library's numerics flags); anything that is not a
// finite number counts as +inf.
__device__ __forceinline__ float pixel_error(float mean, float m2, uint32_t n, float floor)
{
    if (n < 2) return __builtin_inff();
    const float e = sqrtf((m2 / (float)(n - 1)) / (float)n) / (fabsf(mean) + floor);
    return e <= 3.40282347e+38f && e >= 0.0f ? e : __builtin_inff();
}

// err[slot] = max over the slot's pixels inside the image (0 when it has none), and with flag the
// rule: active when n < max && (n < min || !(E <= threshold)).
__global__ void __launch_bounds__(64 * TILES_PER_BLOCK) adapt_error_kernel(const float* __restrict__ mean,
                                                                            const float* __restrict__ m2,
                                                                            const uint32_t* __restrict__ done, SelectArgs sa,
                                                                            float* __restrict__ err, uint32_t* __restrict__ flag)
{
    const int     lane = threadIdx.x & 63;
    const int64_t slot = (int64_t)blockIdx.x * TILES_PER_BLOCK + (threadIdx.x >> 6);
    if (slot >= sa.num_tiles) return;
    const int32_t  tile   = sa.tile_ids ? sa.tile_ids[slot] : (int32_t)slot;
    const uint32_t px     = (uint32_t)((tile % sa.tiles_x) * 8) + compact_bits((uint32_t)lane);
    const uint32_t py     = (uint32_t)((tile / sa.tiles_x) * 8) + compact_bits((uint32_t)lane >> 1);
    const bool     inside = px < (uint32_t)sa.width && py < (uint32_t)sa.height; // as render_tiles_body
    const uint32_t n      = done[slot];
    const size_t   p      = (size_t)slot * 64 + lane;
    float          e      = inside ? pixel_error(mean[p], m2[p], n, sa.floor) : 0.0f;
    for (int off = 32; off > 0; off >>= 1) e = fmaxf(e, __shfl_xor(e, off, 64)); // exact in any order
    if (lane != 0) return;
    err[slot] = e;
    if (flag) flag[slot] = (n < sa.max_samples && (n < sa.min_samples || !(e <= sa.threshold))) ? 1u : 0u;
}

// active[0 .. *n_active) = the flagged slots in queue order (order[j], or j), stable.  One block
// walks the queue 1024 positions at a time: a wave's ballot gives each lane its place in the wave,
// the 16 wave totals in LDS give the wave's place in the step.
__global__ void __launch_bounds__(COMPACT_THREADS) adapt_compact_kernel(const uint32_t* __restrict__ flag,
                                                                         const int32_t* __restrict__ order, int64_t n,
                                                                         int32_t* __restrict__ active, int32_t* __restrict__ n_active)
{
    __shared__ int wave_total[COMPACT_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int       base = 0;
    for (int64_t j0 = 0; j0 < n; j0 += COMPACT_THREADS) {
        const int64_t j    = j0 + tid;
        int64_t       slot = -1;
        if (j < n) slot = order ? (int64_t)order[j] : j;
        const bool     f    = slot >= 0 && slot < n && flag[slot] != 0;
        const uint64_t vote = __ballot(f);
        if (lane == 0) wave_total[wave] = __popcll(vote);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < COMPACT_THREADS / 64; ++w) {
            const int v = wave_total[w];
            before += w < wave ? v : 0;
            total += v;
        }
        if (f) active[base + before + __popcll(vote & ((1ull << lane) - 1ull))] = (int32_t)slot;
        base += total;
        __syncthreads();
    }
    if (tid == 0) *n_active = base;
}

// out of every slot the round does not render (flag 0; flag == nullptr: every slot): sum / done as
// the render kernel's last line writes it (cdivs by (float)i_end), zeros where nothing is done.
__global__ void __launch_bounds__(64 * TILES_PER_BLOCK) adapt_resolve_kernel(const float* __restrict__ sum,
                                                                              const uint32_t* __restrict__ done,
                                                                              const uint32_t* __restrict__ flag, int64_t n,
                                                                              float* __restrict__ out)
{
    const int     lane = threadIdx.x & 63;
    const int64_t slot = (int64_t)blockIdx.x * TILES_PER_BLOCK + (threadIdx.x >> 6);
    if (slot >= n) return;
    if (flag && flag[slot] != 0) return;
    const uint32_t c = done[slot];
    const float*   s = sum + (size_t)slot * 192 + lane;
    float*         o = out + ((size_t)slot * 64 + lane) * 3;
    o[0]             = c ? s[0] / (float)c : 0.0f;
    o[1]             = c ? s[64] / (float)c : 0.0f;
    o[2]             = c ? s[128] / (float)c : 0.0f;
}
} // namespace

static unsigned tile_blocks(int64_t n) { return (unsigned)((n + TILES_PER_BLOCK - 1) / TILES_PER_BLOCK); }

hipError_t launch_adapt_select(const AdaptArgs& ad, const SelectArgs& sa, float* err, uint32_t* flag, hipStream_t stream)
{
    hipLaunchKernelGGL(adapt_error_kernel, dim3(tile_blocks(sa.num_tiles)), dim3(64 * TILES_PER_BLOCK), 0, stream, ad.mean, ad.m2,
                       ad.done, sa, err, flag);
    return hipGetLastError();
}

hipError_t launch_adapt_compact(const AdaptArgs& ad, const int32_t* order, int64_t n_tiles, hipStream_t stream)
{
    hipLaunchKernelGGL(adapt_compact_kernel, dim3(1), dim3(COMPACT_THREADS), 0, stream, ad.flag, order, n_tiles, ad.active,
                       ad.n_active);
    return hipGetLastError();
}

hipError_t launch_adapt_resolve(const ResumeArgs& res, const AdaptArgs& ad, bool skip_active, int64_t n_tiles, float* out,
                                hipStream_t stream)
{
    hipLaunchKernelGGL(adapt_resolve_kernel, dim3(tile_blocks(n_tiles)), dim3(64 * TILES_PER_BLOCK), 0, stream, res.sum, ad.done,
                       skip_active ? ad.flag : nullptr, n_tiles, out);
    return hipGetLastError();
}
} // namespace spd
