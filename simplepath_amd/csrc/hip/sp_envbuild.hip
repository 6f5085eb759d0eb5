// sp_envbuild.hip -- the image light's tables on the device.
//
// What the ImageBasedEnvironmentLight constructor computes from its pixels, stage by stage as
// sph::build_env_map (sp_envmap.cpp) restates it on the host, with the same float operations in the
// same order: this file is built without FP contraction, division is IEEE, and sin / fmod / round
// are the device libm of sp_libm.h, which equals glibc bit for bit.  The two are kept apart on
// purpose: the host file is what this one is tested against (sp_scene_env_check).
//
//   eb_clamp    one lane per texel: modify_image, into the float4 radiance image
//   eb_func     one lane per (u, v) of the 2w x 2h grid: luminance x sin(theta), abs, into cond_func
//   eb_rows     Distribution1D per row.  cdf[i] = cdf[i-1] + func[i-1] * 1.0f / n is a float
//               recurrence that may not be re-associated, so the parallelism is across rows: a lane
//               owns a row and walks it left to right.  A block of 64 lanes stages ROWS x COLS tiles
//               through LDS: the lanes read COLS consecutive floats of each row (coalesced), divide
//               by n (the parallel part), and store them at a pitch of COLS + 1 words, so that the
//               ROWS lanes which then add along their own rows read ROWS different banks (tiles of
//               16 rows: the stage is bound by the latency of this chain, and twice the blocks of 32
//               rows halve it).  The
//               running sums go back through the same tile.  The second half divides by the row's
//               integral with the constructor's one-slot shift, cdf[i] = cdf[i+1] / I, in place:
//               tiles left to right, a tile's loads all done (a barrier) before its stores, which
//               reach back only one slot into what the tile before it has already read.
//               The marginal is the same kernel on cond_int as one row.
//   eb_ordered  !(cdf[i-1] <= cdf[i]) anywhere (NaN fails) sets one flag word with a vector atomic
//   eb_guide    one lane per guide entry: the host's running `while (i < n && !(cdf[i] > v)) ++i` over
//               a non-decreasing cdf is the first i with cdf[i] > v, found by binary search
// Every hand-off is a kernel boundary on the null stream; the host reads the flag and the
// marginal's integral once.
#include "sp_envbuild.hpp"
#include "sp_devbuild.hpp"
#include "../common/sp_libm.h"

namespace spe {

EnvSizes env_sizes(int w, int h)
{
    EnvSizes s{};
    s.nu         = 2 * w;
    s.nv         = 2 * h;
    s.texels     = (size_t)w * (size_t)h;
    s.func       = (size_t)s.nu * (size_t)s.nv;
    s.cdf        = ((size_t)s.nu + 1) * (size_t)s.nv;
    s.rows       = (size_t)s.nv;
    s.marg_cdf   = (size_t)s.nv + 1;
    auto bits    = [](size_t n) { int b = 0; while (((size_t)1 << b) < n && b < 16) ++b; return b; };
    s.cond_bits  = bits((size_t)s.nu);
    s.marg_bits  = bits((size_t)s.nv);
    s.cond_guide = (((size_t)1 << s.cond_bits) + 1) * (size_t)s.nv;
    s.marg_guide = ((size_t)1 << s.marg_bits) + 1;
    return s;
}

namespace {

using spb::BLOCK;
using spb::blocks_for;

#ifndef SP_ENV_ROWS
#define SP_ENV_ROWS 16 // rows of a tile of eb_rows (a comparison build may give another: DESIGN.md §29)
#endif
constexpr int ROWS = SP_ENV_ROWS, COLS = 64, PITCH = COLS + 1; // eb_rows: a tile, and its row pitch in LDS words
static_assert(ROWS >= 1 && ROWS <= 64, "a lane per row of a tile");
constexpr float k_max_less_than_one = 0x1.fffffep-1f;

// NaN as SSE arithmetic leaves it, which the host's tables hold: an operation with a NaN operand
// returns the first NaN operand, quieted, and an invalid one (inf - inf, 0 * inf, inf / inf) the
// default NaN with its sign bit set.  The fast path is one test of the result.
__device__ inline float x86_nan(float r, float a, float b)
{
    if (!spm::is_nan_bits(r)) return r;
    if (spm::is_nan_bits(a)) return spm::x86_quiet(a);
    if (spm::is_nan_bits(b)) return spm::x86_quiet(b);
    return spm::x86_default_nan();
}
__device__ inline float xadd(float a, float b) { return x86_nan(a + b, a, b); }
__device__ inline float xmul(float a, float b) { return x86_nan(a * b, a, b); }
__device__ inline float xdiv(float a, float b) { return x86_nan(a / b, a, b); }

__device__ inline float relative_luminance(float r, float g, float b)
{
    return xadd(xadd(xmul(0.2126f, r), xmul(0.7152f, g)), xmul(0.0722f, b));
}
__device__ inline bool is_inf(float x) { return spm::abs_f(x) == INFINITY; }

__global__ __launch_bounds__(BLOCK) void eb_clamp(const float* __restrict__ pixels, uint64_t texels, float maxr,
                                                  float4* __restrict__ radiance)
{
    const uint64_t p = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= texels) return;
    float c0 = pixels[3 * p], c1 = pixels[3 * p + 1], c2 = pixels[3 * p + 2];
    if (is_inf(c0)) c0 = maxr;
    if (is_inf(c1)) c1 = maxr;
    if (is_inf(c2)) c2 = maxr;
    if (relative_luminance(c0, c1, c2) > maxr) {
        const int mi = (c0 > c1) ? ((c0 > c2) ? 0 : 2) : ((c1 > c2) ? 1 : 2); // index_of_max
        float     d  = mi == 0 ? c0 : (mi == 1 ? c1 : c2);                    // c[mi], which changes once i passes mi
        c0 = xdiv(xmul(c0, maxr), d);
        if (mi == 0) d = c0;
        c1 = xdiv(xmul(c1, maxr), d);
        if (mi == 1) d = c1;
        c2 = xdiv(xmul(c2, maxr), d);
    }
    radiance[p] = make_float4(c0, c1, c2, 0.0f);
}

__global__ __launch_bounds__(BLOCK) void eb_func(const float4* __restrict__ radiance, int w, int h, float maxr,
                                                 float* __restrict__ cond_func)
{
    const uint32_t width = 2u * (uint32_t)w, height = 2u * (uint32_t)h;
    const uint64_t k     = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (k >= (uint64_t)width * height) return;
    const uint32_t v = (uint32_t)(k / width), u = (uint32_t)(k % width);
    const float    pi        = 3.14159265358979323846f;
    const float    vp        = (static_cast<float>(v) + 0.5f) / static_cast<float>(height);
    const float    sin_theta = spm::lm_sinf(pi * (static_cast<float>(v) + 0.5f) / static_cast<float>(height));
    const float    up        = (static_cast<float>(u) + 0.5f) / static_cast<float>(width);
    // nearest_texel: RemapWrap / RemapClamp + sample_nearest_neighbor
    const float    s  = spm::fmod1(1.0f + spm::fmod1(up));
    const float    t  = (vp < 0.0f) ? 0.0f : ((k_max_less_than_one < vp) ? k_max_less_than_one : vp);
    const float    fu = spm::round_f(s * static_cast<float>(w));
    const float    fv = spm::round_f(t * static_cast<float>(h));
    const uint32_t x  = min(static_cast<uint32_t>(fu), static_cast<uint32_t>(w - 1));
    const uint32_t y  = min(static_cast<uint32_t>(fv), static_cast<uint32_t>(h - 1));
    const float4   c  = radiance[(uint64_t)y * (uint32_t)w + x];
    float          f  = relative_luminance(c.x, c.y, c.z);
    f = xmul(f, sin_theta);
    if (is_inf(f)) f = maxr;
    f = (maxr < f) ? maxr : f; // std::min
    cond_func[k] = spm::abs_f(f);
}

// Distribution1D of `rows` rows of n values: func = abs(src) (written when WRITE_FUNC; the rows of the
// conditional are their own abs already), cdf of n + 1 per row, the integral per row.  64 lanes.
template <bool WRITE_FUNC>
__global__ __launch_bounds__(64) void eb_rows(const float* __restrict__ src, float* __restrict__ func, float* cdf,
                                              float* __restrict__ integral, uint32_t rows, uint32_t n)
{
    __shared__ float tile[ROWS * PITCH];
    __shared__ float row_int[ROWS];
    const uint32_t t  = threadIdx.x;
    const uint32_t r0 = blockIdx.x * ROWS;
    const uint32_t nr = min((uint32_t)ROWS, rows - r0);
    const float    fn = static_cast<float>(n);
    float          acc = 0.0f;
    if (t < nr) cdf[(uint64_t)(r0 + t) * (n + 1ull)] = 0.0f;
    for (uint32_t c0 = 0; c0 < n; c0 += COLS) {
        const uint32_t nc = min((uint32_t)COLS, n - c0);
        if (t < nc)
            for (uint32_t r = 0; r < nr; ++r) {
                const uint64_t at = (uint64_t)(r0 + r) * n + c0 + t;
                const float    f  = spm::abs_f(src[at]);
                if (WRITE_FUNC) func[at] = f;
                tile[r * PITCH + t] = xdiv(f * 1.0f, fn);
            }
        __syncthreads();
        if (t < nr)
            for (uint32_t c = 0; c < nc; ++c) {
                acc                 = xadd(acc, tile[t * PITCH + c]);
                tile[t * PITCH + c] = acc;
            }
        __syncthreads();
        if (t < nc)
            for (uint32_t r = 0; r < nr; ++r) cdf[(uint64_t)(r0 + r) * (n + 1ull) + c0 + 1 + t] = tile[r * PITCH + t];
        __syncthreads();
    }
    if (t < nr) {
        row_int[t]        = acc;
        integral[r0 + t] = acc;
    }
    __threadfence_block();
    __syncthreads();
    // I == 0: cdf[i] = i / n for i in 1..n.  Else cdf[i] = cdf[i + 1] / I for i < n, and cdf[n] stays I.
    for (uint32_t c0 = 0; c0 < n; c0 += COLS) {
        const uint32_t nc = min((uint32_t)COLS, n - c0);
        const uint32_t j  = c0 + 1 + t; // the slot this lane reads
        if (t < nc)
            for (uint32_t r = 0; r < nr; ++r) {
                const float I = row_int[r];
                const float raw = cdf[(uint64_t)(r0 + r) * (n + 1ull) + j];
                tile[r * PITCH + t] = (I == 0.0f) ? static_cast<float>(j) / fn : xdiv(raw, I);
            }
        __syncthreads();
        if (t < nc)
            for (uint32_t r = 0; r < nr; ++r) {
                const uint32_t to = (row_int[r] == 0.0f) ? j : j - 1;
                cdf[(uint64_t)(r0 + r) * (n + 1ull) + to] = tile[r * PITCH + t];
            }
        __threadfence_block();
        __syncthreads();
    }
}

// cdf[0..n-1] of every row non-decreasing?  one lane per entry; a failure (NaN too) sets *flag
__global__ __launch_bounds__(BLOCK) void eb_ordered(const float* __restrict__ cdf, uint32_t rows, uint32_t n, uint32_t* flag)
{
    const uint64_t k = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (k >= (uint64_t)rows * n) return;
    const uint32_t row = (uint32_t)(k / n), i = (uint32_t)(k % n);
    if (i == 0) return;
    const float* c = cdf + (uint64_t)row * (n + 1ull);
    if (!(c[i - 1] <= c[i])) atomicOr(flag, 1u);
}

// guide[b] = first i < n with cdf[i] > b / 2^bits, clamped to n - 1; one lane per entry
__global__ __launch_bounds__(BLOCK) void eb_guide(const float* __restrict__ cdf, uint32_t rows, uint32_t n, int bits,
                                                  uint32_t* __restrict__ guide)
{
    const uint32_t g1 = (1u << bits) + 1u;
    const uint64_t k  = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (k >= (uint64_t)rows * g1) return;
    const uint32_t row = (uint32_t)(k / g1), b = (uint32_t)(k % g1);
    const float    v   = static_cast<float>(b) * (1.0f / static_cast<float>(1u << bits)); // exact: b / 2^bits
    const float*   c   = cdf + (uint64_t)row * (n + 1ull);
    uint32_t       lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (c[mid] > v) hi = mid;
        else lo = mid + 1;
    }
    guide[k] = min(lo, n - 1u);
}

} // namespace

int build_env_device(const EnvBuildIn& in, EnvBuildOut& out, EnvBuildStats& st, std::string& err, bool timed)
{
    st  = EnvBuildStats{};
    out = EnvBuildOut{};
    const auto start = spb::Stage::clock::now();
    spb::Stage stage("device environment build", err, timed);
    if (in.w <= 0 || in.h <= 0 || in.w > 32767 || in.h > 32767) return stage.refuse("the image size is out of range", SP_ERR_UNSUPPORTED);
    const EnvSizes z = env_sizes(in.w, in.h);
    if (z.func / BLOCK + 1 > 0x7fffffffull || z.cond_guide / BLOCK + 1 > 0x7fffffffull)
        return stage.refuse("the image is too large for one launch", SP_ERR_UNSUPPORTED);

    const float* d_pixels = in.d_pixels;
    uint32_t*    d_ctr    = nullptr; // [0] the order flag, [1] the marginal's integral
    SPB_HIP(stage.mem.get(&d_ctr, 4));
    SPB_HIP(hipMemset(d_ctr, 0, 16));
    if (!d_pixels) {
        float* up = nullptr;
        SPB_HIP(stage.mem.get(&up, z.texels * 3));
        SPB_HIP(hipMemcpy(up, in.h_pixels, z.texels * 3 * sizeof(float), hipMemcpyHostToDevice));
        d_pixels = up;
    }
    stage.lap(st.ms_upload);

    const uint32_t nu = (uint32_t)z.nu, nv = (uint32_t)z.nv;
    hipLaunchKernelGGL(eb_clamp, dim3(blocks_for(z.texels)), dim3(BLOCK), 0, 0, d_pixels, (uint64_t)z.texels, in.max_radiance, in.radiance);
    SPB_HIP(hipGetLastError());
    stage.lap(st.ms_clamp);

    hipLaunchKernelGGL(eb_func, dim3(blocks_for(z.func)), dim3(BLOCK), 0, 0, in.radiance, in.w, in.h, in.max_radiance, in.cond_func);
    SPB_HIP(hipGetLastError());
    stage.lap(st.ms_func);

    hipLaunchKernelGGL(eb_rows<false>, dim3((nv + ROWS - 1) / ROWS), dim3(64), 0, 0, in.cond_func, (float*)nullptr, in.cond_cdf,
                       in.cond_int, nv, nu);
    SPB_HIP(hipGetLastError());
    stage.lap(st.ms_rows);

    hipLaunchKernelGGL(eb_rows<true>, dim3(1), dim3(64), 0, 0, in.cond_int, in.marg_func, in.marg_cdf,
                       reinterpret_cast<float*>(d_ctr + 1), 1u, nv);
    SPB_HIP(hipGetLastError());
    stage.lap(st.ms_marginal);

    hipLaunchKernelGGL(eb_ordered, dim3(blocks_for(nv)), dim3(BLOCK), 0, 0, in.marg_cdf, 1u, nv, d_ctr);
    hipLaunchKernelGGL(eb_ordered, dim3(blocks_for(z.func)), dim3(BLOCK), 0, 0, in.cond_cdf, nv, nu, d_ctr);
    SPB_HIP(hipGetLastError());
    uint32_t ctr[4] = {};
    SPB_HIP(hipMemcpy(ctr, d_ctr, 16, hipMemcpyDeviceToHost)); // (waits for the null stream)
    out.guided   = ctr[0] == 0;
    out.marg_int = spm::u2f(ctr[1]);
    if (out.guided && in.cond_guide && in.marg_guide) {
        hipLaunchKernelGGL(eb_guide, dim3(blocks_for(z.marg_guide)), dim3(BLOCK), 0, 0, in.marg_cdf, 1u, nv, z.marg_bits, in.marg_guide);
        hipLaunchKernelGGL(eb_guide, dim3(blocks_for(z.cond_guide)), dim3(BLOCK), 0, 0, in.cond_cdf, nv, nu, z.cond_bits, in.cond_guide);
        SPB_HIP(hipGetLastError());
    }
    SPB_HIP(hipDeviceSynchronize());
    stage.lap(st.ms_guides);
    st.peak_bytes = stage.mem.peak;
    st.ms_total   = std::chrono::duration<double, std::milli>(spb::Stage::clock::now() - start).count();
    return SP_OK;
}

} // namespace spe
