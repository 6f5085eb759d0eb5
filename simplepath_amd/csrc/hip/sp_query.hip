// sp_query.hip -- ray queries on the resident scene (sp_scene_trace_rays): the reference's
// Scene::intersect (base/Scene.h:74) and Scene::intersect_p (base/Scene.h:79) for rays the caller
// brings, one lane per ray.
//
//   sp_query_closest_kernel<NORMALS>  scene_intersect -> one 32-byte hit record per ray, and with
//                                     NORMALS finish_hit's shading normal
//   sp_query_any_kernel               geometry_any    -> one word per ray
//
// The walks are the render kernels' own (sp_path.hpp), called with the ray's limits: whatever walk
// the upload chose (binary with the LDS stack, parent links, 8-wide) answers the query, so a hit is
// the hit an integrator's ray would have found.  The kernels are not persistent: rays cost roughly
// alike and their order is the caller's.  A ray is two 16-byte loads, a hit two 16-byte stores.
//
// Rays no integrator makes.  Two kinds are answered before any walk:
//   * a NaN limit, or an origin or direction component that is not finite: a miss (the reference's
//     triangle test would accept such a ray, since every comparison it rejects by is false for NaN);
//   * a zero direction: a miss, which is what every leaf test returns for it (the triangle's
//     denominator and the plane's d.y are 0, the sphere's discriminant is not positive).
// Every other ray is walked with its own limits, tmax = +inf included, by the walks' NAN_SAFE form
// (sp_path.hpp wide_visit): the 8-wide walk orders a node's children by entry distances below
// FLT_MAX, and a caller's ray can make that distance NaN (a direction component whose reciprocal is
// infinite, the origin exactly in a box plane: 0 * inf) or +inf (tmax = +inf, the ray outside a
// slab it runs parallel to).  Such a child is entered like any other.
#include "sp_path.hpp"
#include "sp_query.hpp"

namespace spd {

static_assert(sizeof(sp_ray) == 32 && sizeof(sp_ray_hit) == 32, "the records are two 16-byte words");

struct QueryRay {
    Ray   ray;
    float tmin, tmax; // the caller's limits
    bool  walk;       // false: answered as a miss without a walk (see above)
};

__device__ __forceinline__ bool finite_bits(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// lanes past num_rays load nothing and walk nothing
__device__ __forceinline__ QueryRay query_ray(const QueryArgs& a, int64_t i)
{
    QueryRay q;
    q.ray.o = mk(0.0f, 0.0f, 0.0f);
    q.ray.d = mk(0.0f, 0.0f, 0.0f);
    q.tmin  = 0.0f;
    q.tmax  = 0.0f;
    q.walk  = false;
    if (i >= a.num_rays) return q;
    const float4* p  = reinterpret_cast<const float4*>(a.rays + i);
    const float4  r0 = p[0], r1 = p[1]; // {o, tmin}, {d, tmax}
    q.ray.o = mk(r0.x, r0.y, r0.z);
    q.ray.d = mk(r1.x, r1.y, r1.z);
    q.tmin  = r0.w;
    q.tmax  = r1.w;
    const bool finite = finite_bits(r0.x) && finite_bits(r0.y) && finite_bits(r0.z) && finite_bits(r1.x) && finite_bits(r1.y) &&
                        finite_bits(r1.z);
    const bool zero   = r1.x == 0.0f && r1.y == 0.0f && r1.z == 0.0f;
    q.walk            = finite && !zero && r0.w == r0.w && r1.w == r1.w;
    return q;
}

// one atomic per wave; every lane of the wave reaches the ballot
__device__ __forceinline__ void count_hits(unsigned long long* counter, bool hit)
{
    if (!counter) return; // kernel argument: uniform
    const unsigned long long n = (unsigned long long)__popcll(__ballot(hit));
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(counter, n);
}

// Waves per SIMD requested: the 7 (closest hit) and 8 (any hit) these kernels had before the one-exit
// node visit, whose eight slots in flight would cost each a step; nothing spills.
template <bool NORMALS>
__global__ void __launch_bounds__(QUERY_BLOCK, 7) sp_query_closest_kernel(Scene sc, QueryArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int tid  = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    int       rs_words = 0;
    if constexpr (NORMALS) { // the shading kernels' LDS copy of the RSQRTSS table (sp_mega.hpp)
        rs_words = rsqrt_words(sc);
        for (int i = tid; i < rs_words; i += QUERY_BLOCK) lds[i] = sc.rsqrt_entries[i];
        __syncthreads();
    }
    const Stack    st{ lds + rs_words + wave * sc.stack_words * 64, lane, sc.stack_depth };
    const int64_t  i = (int64_t)blockIdx.x * QUERY_BLOCK + tid;
    const QueryRay q = query_ray(a, i);

    Hit h;
    h.t     = q.tmax;
    h.code  = 0xffffffffu;
    h.beta  = 0.0f;
    h.gamma = 0.0f;
    if (q.walk) h = scene_intersect<true>(sc, q.ray, q.tmin, q.tmax, st);
    const bool hit = h.code != 0xffffffffu;
    if (i < a.num_rays) {
        int32_t kind = -1, index = -1, material = -1;
        float   t = q.tmax, beta = 0.0f, gamma = 0.0f;
        f3      n = mk(0.0f, 0.0f, 0.0f);
        if (hit) {
            kind  = (int32_t)(h.code >> CODE_SHIFT);
            index = (int32_t)(h.code & CODE_MASK);
            t     = h.t;
            if (kind == (int32_t)KIND_TRI) {
                beta  = h.beta;
                gamma = h.gamma;
            }
            if constexpr (NORMALS) {
                const Isect is = finish_hit(sc, h, q.ray, Rsq{ lds });
                n              = is.n;
                material       = is.material;
            } else {
                material = kind == (int32_t)KIND_TRI ? sc.tri_material[index] : sc.shapes[index].material;
            }
        }
        float4* o = reinterpret_cast<float4*>(a.hits + i);
        o[0]      = make_float4(t, __int_as_float(kind), __int_as_float(index), __int_as_float(material));
        o[1]      = make_float4(beta, gamma, 0.0f, 0.0f);
        if constexpr (NORMALS) a.normals[i] = make_float4(n.x, n.y, n.z, 0.0f);
    }
    count_hits(a.hit_count, hit);
}

__global__ void __launch_bounds__(QUERY_BLOCK, 8) sp_query_any_kernel(Scene sc, QueryArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int      lane = threadIdx.x & 63;
    const int      wave = threadIdx.x >> 6;
    const Stack    st{ lds + wave * sc.any_stack_words * 64, lane, sc.any_stack_words };
    const int64_t  i = (int64_t)blockIdx.x * QUERY_BLOCK + threadIdx.x;
    const QueryRay q = query_ray(a, i);
    const bool     occ = q.walk ? geometry_any<true>(sc, q.ray, q.tmin, q.tmax, st) : false;
    if (i < a.num_rays) a.occluded[i] = occ ? 1u : 0u;
    count_hits(a.hit_count, occ);
}

// ---------------------------------------------------------------------------- host side
size_t query_lds_bytes(const Scene& sc, bool any_hit, bool normals)
{
    const size_t words = (size_t)(any_hit ? sc.any_stack_words : sc.stack_words);
    return (size_t)(QUERY_BLOCK / 64) * words * 64 * 4 + (normals ? (size_t)rsqrt_words(sc) * 4 : 0);
}

static dim3 query_grid(const QueryArgs& a) { return dim3((unsigned)((a.num_rays + QUERY_BLOCK - 1) / QUERY_BLOCK)); }

hipError_t launch_query_closest(const Scene& sc, const QueryArgs& a, size_t lds_bytes, hipStream_t stream)
{
    if (a.normals) hipLaunchKernelGGL(sp_query_closest_kernel<true>, query_grid(a), dim3(QUERY_BLOCK), lds_bytes, stream, sc, a);
    else hipLaunchKernelGGL(sp_query_closest_kernel<false>, query_grid(a), dim3(QUERY_BLOCK), lds_bytes, stream, sc, a);
    return hipGetLastError();
}

hipError_t launch_query_any(const Scene& sc, const QueryArgs& a, size_t lds_bytes, hipStream_t stream)
{
    hipLaunchKernelGGL(sp_query_any_kernel, query_grid(a), dim3(QUERY_BLOCK), lds_bytes, stream, sc, a);
    return hipGetLastError();
}

} // namespace spd
