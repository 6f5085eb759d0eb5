// sp_features.hip -- the render's camera samples, exported and reduced (sp_scene_camera_rays,
// sp_scene_features): the guide images a denoiser or compositor wants beside a Monte-Carlo frame,
// taken on exactly the sub-pixel positions the render integrates.
//
//   sp_camera_rays_kernel   tail_camera_ray(px, py, i) -> one 32-byte sp_ray per pixel and sample
//   sp_features_kernel<F>   per pixel, over its samples i = 0 .. n - 1 in order: the camera ray,
//                           scene_intersect with the integrators' limits, (F) finish_hit; the sums
//                           stay in registers and every output is written once, after the loop
//
// One lane owns one pixel and one wave one tile slot, in the megakernel's Morton lane order, so the
// outputs are tile-packed like the image.  The grid is plain (a block of four waves takes four
// consecutive slots): tiles cost roughly alike, one closest-hit walk per sample and no shading.
//
// Geometry only, as a ray query: lights are not intersected, so a sphere light in front of geometry
// is not in the buffers.  The walk is the render's scene_intersect in the render's own form (not
// the ray queries' NAN_SAFE form: a camera ray is a ray an integrator makes), whichever accelerator
// the upload chose.
//
// The reduction.  H = the samples that hit, in sample order.  A sum takes its first term as it is
// and adds the others in order ((x_0 + x_1) + x_2 ...; no 0 + x_0, which would turn a -0 into +0),
// float32, no contraction; then one division by (float)|H|.  |H| = 0 writes +0.
#include "sp_mega.hpp"
#include "sp_features.hpp"

namespace spd {

static_assert(sizeof(sp_ray) == 32, "the record is two 16-byte words");

// the pixel of (tile slot, lane); false: outside the image (a clipped border tile, or a device
// list's id outside the frame: unsigned compares, as the megakernel's)
__device__ __forceinline__ bool feature_pixel(const Scene& sc, const int32_t* tile_ids, int32_t tiles_x, int64_t slot, int lane,
                                              uint32_t& px, uint32_t& py)
{
    const int32_t tile = tile_ids ? tile_ids[slot] : (int32_t)slot;
    px                 = (uint32_t)((tile % tiles_x) * 8) + morton_decode_1((uint32_t)lane);
    py                 = (uint32_t)((tile / tiles_x) * 8) + morton_decode_1((uint32_t)lane >> 1);
    return px < (uint32_t)sc.width && py < (uint32_t)sc.height;
}

// the block's LDS copy of the RSQRTSS table (sp_mega.hpp); returns its words
__device__ __forceinline__ int feature_rsqrt_lds(const Scene& sc, uint32_t* lds, int tid)
{
    const int rs_words = rsqrt_words(sc);
    for (int i = tid; i < rs_words; i += FEATURE_BLOCK) lds[i] = sc.rsqrt_entries[i];
    __syncthreads();
    return rs_words;
}

// Item w of the grid's waves is (slot, s) = (w / num_samples, w % num_samples): record w * 64 + lane.
__global__ void __launch_bounds__(FEATURE_BLOCK) sp_camera_rays_kernel(Scene sc, CameraRayArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int tid  = threadIdx.x;
    const int lane = tid & 63;
    feature_rsqrt_lds(sc, lds, tid);
    const Rsq     q{ lds };
    const int64_t item = (int64_t)blockIdx.x * (FEATURE_BLOCK / 64) + (tid >> 6);
    if (item >= a.num_tiles * (int64_t)a.num_samples) return; // (after the block's only barrier)
    const int64_t  slot = item / a.num_samples;
    const uint32_t s    = (uint32_t)(item % a.num_samples);
    uint32_t       px, py;
    float4         r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = r0; // outside: a miss without a walk for sp_scene_trace_rays
    if (feature_pixel(sc, a.tile_ids, a.tiles_x, slot, lane, px, py)) {
        const Ray ray = tail_camera_ray(sc, px, py, a.first_sample + s, q);
        r0            = make_float4(ray.o.x, ray.o.y, ray.o.z, k_ray_epsilon);
        r1            = make_float4(ray.d.x, ray.d.y, ray.d.z, k_infinite);
    }
    float4* o = reinterpret_cast<float4*>(a.rays + item * 64 + lane);
    o[0]      = r0;
    o[1]      = r1;
}

// a sum's next term: the first as it is (see the head of this file)
__device__ __forceinline__ float sum_next(float sum, float x, bool first) { return first ? x : sum + x; }

// the wave's total of v in every lane; every lane of the wave reaches it
__device__ __forceinline__ unsigned long long wave_total(uint32_t v)
{
    unsigned long long t = v;
    for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
    return t;
}

// FINISH: a normal or an albedo is wanted, so every hit is finished (finish_hit).  Without it a hit
// costs the walk alone, and sample 0's material is read from the primitive as a ray query does.
// Waves per SIMD requested: 4, the DirectLighting megakernel's.  The sums, the count, sample 0's ids
// and the pixel are live across the walk on top of what the closest-hit query keeps: at 5 and 6 the
// FINISH form spills 16 and 76 bytes per lane to scratch, at 4 it takes 99 VGPRs and none
// (DESIGN.md section 31).
template <bool FINISH>
__global__ void __launch_bounds__(FEATURE_BLOCK, 4) sp_features_kernel(Scene sc, FeatureArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int tid      = threadIdx.x;
    const int lane     = tid & 63;
    const int wave     = tid >> 6;
    const int rs_words = feature_rsqrt_lds(sc, lds, tid);
    const Rsq     q{ lds };
    const Stack   st{ lds + rs_words + wave * sc.stack_words * 64, lane, sc.stack_depth };
    const int64_t slot = (int64_t)blockIdx.x * (FEATURE_BLOCK / 64) + wave;
    const bool    live = slot < a.num_tiles; // wave-uniform; a wave past the list still reaches wave_total

    uint32_t n = 0, px = 0, py = 0;
    bool     inside = false;
    if (live) {
        n      = a.tile_samples ? a.tile_samples[slot] : a.spp;
        inside = feature_pixel(sc, a.tile_ids, a.tiles_x, slot, lane, px, py);
    }
    uint32_t cnt = 0;
    int32_t  kind0 = -1, index0 = -1, material0 = -1;
    float    tsum = 0.0f;
    f3       nsum = mk(0.0f, 0.0f, 0.0f);
    rgb      asum = mkc(0, 0, 0);
    if (inside) {
        for (uint32_t i = 0; i < n; ++i) {
            const Ray ray = tail_camera_ray(sc, px, py, i, q);
            const Hit h   = scene_intersect(sc, ray, k_ray_epsilon, k_infinite, st);
            if (h.code == 0xffffffffu) continue;
            const bool first = cnt == 0;
            tsum             = sum_next(tsum, h.t, first);
            int32_t material;
            if constexpr (FINISH) {
                const Isect is = finish_hit(sc, h, ray, q);
                material       = is.material;
                nsum.x         = sum_next(nsum.x, is.n.x, first);
                nsum.y         = sum_next(nsum.y, is.n.y, first);
                nsum.z         = sum_next(nsum.z, is.n.z, first);
                if (a.albedo) { // kernel argument: uniform
                    const Material* m = sc.materials + material;
                    if (m->kind == SP_MAT_CLEARCOAT) m = sc.materials + m->base; // (never a clearcoat itself)
                    const rgb c = m->lambert_albedo;
                    asum.r      = sum_next(asum.r, c.r * 3.14159274f, first);
                    asum.g      = sum_next(asum.g, c.g * 3.14159274f, first);
                    asum.b      = sum_next(asum.b, c.b * 3.14159274f, first);
                }
            }
            if (i == 0) {
                kind0  = (int32_t)(h.code >> CODE_SHIFT);
                index0 = (int32_t)(h.code & CODE_MASK);
                if constexpr (FINISH) material0 = material;
                else material0 = kind0 == (int32_t)KIND_TRI ? sc.tri_material[index0] : sc.shapes[index0].material;
            }
            ++cnt;
        }
    }
    if (live) {
        const size_t p  = (size_t)slot * 64 + lane;
        const bool   any = cnt != 0;
        const float  fh  = (float)cnt;
        if (a.ids) a.ids[p] = make_int4(kind0, index0, material0, (int32_t)cnt);
        if (a.coverage) a.coverage[p] = any ? fh / (float)n : 0.0f;
        if (a.depth) a.depth[p] = any ? tsum / fh : 0.0f;
        if constexpr (FINISH) {
            if (a.normal) {
                a.normal[p * 3 + 0] = any ? nsum.x / fh : 0.0f;
                a.normal[p * 3 + 1] = any ? nsum.y / fh : 0.0f;
                a.normal[p * 3 + 2] = any ? nsum.z / fh : 0.0f;
            }
            if (a.albedo) {
                a.albedo[p * 3 + 0] = any ? asum.r / fh : 0.0f;
                a.albedo[p * 3 + 1] = any ? asum.g / fh : 0.0f;
                a.albedo[p * 3 + 2] = any ? asum.b / fh : 0.0f;
            }
        }
    }
    if (a.counters) { // kernel argument: uniform; one pair of atomics per wave
        const unsigned long long rays = wave_total(inside ? n : 0u), hits = wave_total(cnt);
        if (lane == 0 && rays) {
            atomicAdd(a.counters + 0, rays);
            atomicAdd(a.counters + 1, hits);
        }
    }
}

// ---------------------------------------------------------------------------- host side
size_t feature_lds_bytes(const Scene& sc)
{
    return (size_t)rsqrt_words(sc) * 4 + (size_t)(FEATURE_BLOCK / 64) * sc.stack_words * 64 * 4;
}

static dim3 wave_grid(int64_t waves) { return dim3((unsigned)((waves + FEATURE_BLOCK / 64 - 1) / (FEATURE_BLOCK / 64))); }

hipError_t launch_camera_rays(const Scene& sc, const CameraRayArgs& a, hipStream_t stream)
{
    hipLaunchKernelGGL(sp_camera_rays_kernel, wave_grid(a.num_tiles * (int64_t)a.num_samples), dim3(FEATURE_BLOCK),
                       (size_t)rsqrt_words(sc) * 4, stream, sc, a);
    return hipGetLastError();
}

hipError_t launch_features(const Scene& sc, const FeatureArgs& a, size_t lds_bytes, hipStream_t stream)
{
    if (a.normal || a.albedo) hipLaunchKernelGGL(sp_features_kernel<true>, wave_grid(a.num_tiles), dim3(FEATURE_BLOCK), lds_bytes, stream, sc, a);
    else hipLaunchKernelGGL(sp_features_kernel<false>, wave_grid(a.num_tiles), dim3(FEATURE_BLOCK), lds_bytes, stream, sc, a);
    return hipGetLastError();
}

} // namespace spd
