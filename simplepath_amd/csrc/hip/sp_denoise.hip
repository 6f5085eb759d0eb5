// sp_denoise.hip -- the edge-avoiding a-trous wavelet filter on tile-packed frames (sp_denoiser_run;
// the rule is in include/simplepath_hip.h, its expressions in ../common/sp_denoise.h).
//
//   sp_denoise_map_kernel       slot_of_tile[tile] = the lowest slot that lists the tile (atomicMin)
//   sp_denoise_prepare_kernel   demodulates the colour and packs what the levels read of a pixel into
//                               two 16-byte records: plane[0] {x0, x1, x2, z} and guide {n0, n1, n2, k}
//   sp_denoise_level_kernel     one launch per level (the levels need a device-wide order between
//                               them): 25 taps per pixel from plane[i & 1] into the other plane, or,
//                               for the last level, remodulated into the caller's output
//
// One wave owns one tile slot and one lane one pixel, in the image's Morton lane order: a wave's own
// loads and stores are contiguous runs (1 KiB of records, 768 bytes of output), and a tap costs two
// 16-byte loads per lane.  The depth gain g_p and the divisor m_p are recomputed where they are used
// (one division per level and pixel beside 25 expf) instead of being stored.
//
// The tap's slot.  At steps 1, 2 and 4 a tap lies in the pixel's tile or one of its eight
// neighbours: nine lanes look the 3x3 neighbourhood up in slot_of_tile once per wave, and each lane
// picks by its tap's tile.  From step 8 on the tap keeps the pixel's lane and its tile is the same
// for the whole wave: 25 lanes look the 25 tap tiles up once per wave, and every tap's loads are
// one contiguous run.  The table goes through the LDS (32 words per wave).
//
// A guide that is not given is stored as zeros and its factor (inv_n, inv_k, g) is +0, so its term
// is +0 without a kernel variant per combination of guides.
#include "sp_denoise.hpp"

namespace spd {

using spdn::Accum;
using spdn::Level;
using spdn::Pixel;

struct DenoisePixel {
    int32_t  tx, ty;  // the slot's tile
    uint32_t px, py;
    bool     tile_ok; // the id names a tile of the frame (a device list may hold any word)
    bool     inside;  // ... and the lane's pixel is inside the image
};

__device__ __forceinline__ DenoisePixel denoise_pixel(const DenoiseArgs& a, int64_t slot, int lane)
{
    const int32_t tile = a.tile_ids ? a.tile_ids[slot] : (int32_t)slot;
    DenoisePixel  p;
    p.tile_ok = (uint32_t)tile < (uint32_t)(a.tiles_x * a.tiles_y);
    p.tx      = p.tile_ok ? tile % a.tiles_x : 0;
    p.ty      = p.tile_ok ? tile / a.tiles_x : 0;
    const uint32_t l = (uint32_t)lane;
    p.px      = (uint32_t)p.tx * 8 + ((l & 1u) | ((l >> 1) & 2u) | ((l >> 2) & 4u));
    p.py      = (uint32_t)p.ty * 8 + (((l >> 1) & 1u) | ((l >> 2) & 2u) | ((l >> 3) & 4u));
    p.inside  = p.tile_ok && p.px < (uint32_t)a.width && p.py < (uint32_t)a.height;
    return p;
}

// the wave's total of v in every lane; every lane of the wave reaches it
__device__ __forceinline__ unsigned long long denoise_wave_total(uint32_t v)
{
    unsigned long long t = v;
    for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
    return t;
}

__global__ void __launch_bounds__(DENOISE_BLOCK) sp_denoise_map_kernel(const int32_t* tile_ids, int64_t num_tiles, int32_t total_tiles,
                                                                       uint32_t* slot_of_tile)
{
    const int64_t slot = (int64_t)blockIdx.x * DENOISE_BLOCK + threadIdx.x;
    if (slot >= num_tiles) return;
    const int32_t tile = tile_ids ? tile_ids[slot] : (int32_t)slot;
    // the preset -1 is the largest unsigned word: the minimum of the slots that list the tile replaces it
    if ((uint32_t)tile < (uint32_t)total_tiles) atomicMin(slot_of_tile + tile, (uint32_t)slot);
}

__global__ void __launch_bounds__(DENOISE_BLOCK) sp_denoise_prepare_kernel(DenoiseArgs a)
{
    const int     lane = threadIdx.x & 63;
    const int64_t slot = (int64_t)blockIdx.x * (DENOISE_BLOCK / 64) + (threadIdx.x >> 6);
    if (slot >= a.num_tiles) return; // wave-uniform
    const DenoisePixel p  = denoise_pixel(a, slot, lane);
    const size_t       pi = (size_t)slot * 64 + lane;
    float4 X = make_float4(0.0f, 0.0f, 0.0f, 0.0f), G = X; // outside the image: never read as a tap
    if (p.inside) {
        if (a.normal) G = make_float4(a.normal[pi * 3 + 0], a.normal[pi * 3 + 1], a.normal[pi * 3 + 2], 0.0f);
        if (a.coverage) G.w = a.coverage[pi];
        if (a.depth) X.w = a.depth[pi];
        float c[3] = { a.color[pi * 3 + 0], a.color[pi * 3 + 1], a.color[pi * 3 + 2] };
        if (a.demodulate) // kernel argument: uniform
            for (int ch = 0; ch < 3; ++ch) c[ch] = c[ch] / spdn::albedo_scale(G.w, a.albedo[pi * 3 + ch], a.albedo_floor);
        X.x = c[0];
        X.y = c[1];
        X.z = c[2];
    }
    a.plane[0][pi] = X;
    a.guide[pi]    = G;
    if (a.counters) { // kernel argument: uniform; one atomic per wave
        const unsigned long long n = (unsigned long long)__popcll(__ballot(p.inside));
        if (lane == 0 && n) atomicAdd(a.counters + 0, n);
    }
}

__device__ __forceinline__ Pixel denoise_load(const float4* plane, const float4* guide, size_t i)
{
    const float4 X = plane[i], G = guide[i];
    Pixel        q;
    q.x[0] = X.x; q.x[1] = X.y; q.x[2] = X.z; q.z = X.w;
    q.n[0] = G.x; q.n[1] = G.y; q.n[2] = G.z; q.k = G.w;
    return q;
}

// FAR: the step is a multiple of 8 (see the head of this file).  LAST: the finish is fused in.
// No minimum of waves is asked for: the kernel takes few registers as it is.
template <bool FAR, bool LAST>
__global__ void __launch_bounds__(DENOISE_BLOCK) sp_denoise_level_kernel(DenoiseArgs a, Level L, int src)
{
    constexpr int SIDE = FAR ? 5 : 3, NB = SIDE * SIDE;
    __shared__ int32_t nb[DENOISE_BLOCK / 64][32];
    const int tid  = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    spm::libm_lds_init(tid, DENOISE_BLOCK);
    const int64_t slot = (int64_t)blockIdx.x * (DENOISE_BLOCK / 64) + wave;
    const bool    live = slot < a.num_tiles; // wave-uniform
    DenoisePixel  p{};
    if (live) p = denoise_pixel(a, slot, lane);
    if (lane < NB) {
        int32_t s = -1;
        if (live && p.tile_ok) {
            const int32_t stride = FAR ? (L.step >> 3) : 1;
            const int32_t ntx = p.tx + (lane % SIDE - SIDE / 2) * stride, nty = p.ty + (lane / SIDE - SIDE / 2) * stride;
            if ((uint32_t)ntx < (uint32_t)a.tiles_x && (uint32_t)nty < (uint32_t)a.tiles_y) s = a.slot_of_tile[nty * a.tiles_x + ntx];
        }
        nb[wave][lane] = s; // a slot of the list, below num_tiles, or -1
    }
    __syncthreads(); // the block's only barrier: the libm table and the neighbour slots
    if (!live) return;

    const size_t  pi    = (size_t)slot * 64 + lane;
    const float4* plane = a.plane[src];
    uint32_t      taps  = 0;
    if (p.inside) {
        const Pixel c = denoise_load(plane, a.guide, pi);
        const float g = a.depth ? spdn::depth_gain(c.z, a.sigma_depth, a.depth_floor) : 0.0f;
        Accum       s;
        for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                const int qx = (int)p.px + dx * L.step, qy = (int)p.py + dy * L.step;
                if ((uint32_t)qx >= (uint32_t)a.width || (uint32_t)qy >= (uint32_t)a.height) continue;
                int32_t  sq;
                uint32_t lq;
                if constexpr (FAR) {
                    sq = nb[wave][(dy + 2) * 5 + (dx + 2)];
                    lq = (uint32_t)lane;
                } else { // at most 8 pixels away: the tile or one of its eight neighbours
                    sq = nb[wave][((qy >> 3) - p.ty + 1) * 3 + ((qx >> 3) - p.tx + 1)];
                    lq = spdn::morton_lane((uint32_t)qx, (uint32_t)qy);
                }
                if (sq < 0) continue;
                const Pixel q = denoise_load(plane, a.guide, (size_t)sq * 64 + lq);
                spdn::accumulate(s, spdn::tap_weight(q, c, g, L, spdn::spline(dx + 2) * spdn::spline(dy + 2)), q);
            }
        }
        taps = s.taps;
        float r[3];
        for (int ch = 0; ch < 3; ++ch) r[ch] = spdn::level_result(s, ch, c.x[ch]);
        if constexpr (LAST) {
            for (int ch = 0; ch < 3; ++ch)
                a.out[pi * 3 + ch] = a.demodulate ? r[ch] * spdn::albedo_scale(c.k, a.albedo[pi * 3 + ch], a.albedo_floor) : r[ch];
        } else {
            a.plane[src ^ 1][pi] = make_float4(r[0], r[1], r[2], c.z);
        }
    } else if constexpr (LAST) {
        for (int ch = 0; ch < 3; ++ch) a.out[pi * 3 + ch] = 0.0f;
    }
    if (a.counters) { // kernel argument: uniform; one atomic per wave
        const unsigned long long n = denoise_wave_total(taps);
        if (lane == 0 && n) atomicAdd(a.counters + 1, n);
    }
}

// ---------------------------------------------------------------------------- host side
static dim3 wave_grid(int64_t waves) { return dim3((unsigned)((waves + DENOISE_BLOCK / 64 - 1) / (DENOISE_BLOCK / 64))); }

hipError_t launch_denoise_map(const int32_t* tile_ids, int64_t num_tiles, int32_t total_tiles, int32_t* slot_of_tile, hipStream_t stream)
{
    hipLaunchKernelGGL(sp_denoise_map_kernel, dim3((unsigned)((num_tiles + DENOISE_BLOCK - 1) / DENOISE_BLOCK)), dim3(DENOISE_BLOCK), 0,
                       stream, tile_ids, num_tiles, total_tiles, reinterpret_cast<uint32_t*>(slot_of_tile));
    return hipGetLastError();
}

hipError_t launch_denoise_prepare(const DenoiseArgs& a, hipStream_t stream)
{
    hipLaunchKernelGGL(sp_denoise_prepare_kernel, wave_grid(a.num_tiles), dim3(DENOISE_BLOCK), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_denoise_level(const DenoiseArgs& a, const Level& L, int i, int levels, hipStream_t stream)
{
    const bool far = L.step >= 8, last = i == levels - 1;
    const dim3 grid = wave_grid(a.num_tiles), block(DENOISE_BLOCK);
    const int  src  = i & 1;
    if (far && last) hipLaunchKernelGGL((sp_denoise_level_kernel<true, true>), grid, block, 0, stream, a, L, src);
    else if (far) hipLaunchKernelGGL((sp_denoise_level_kernel<true, false>), grid, block, 0, stream, a, L, src);
    else if (last) hipLaunchKernelGGL((sp_denoise_level_kernel<false, true>), grid, block, 0, stream, a, L, src);
    else hipLaunchKernelGGL((sp_denoise_level_kernel<false, false>), grid, block, 0, stream, a, L, src);
    return hipGetLastError();
}

} // namespace spd
