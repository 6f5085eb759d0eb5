// wide_visit_units.hip -- the device's wide_visit (sp_path.hpp: the node fetch and spw::visit, with
// the library's numeric and device flags) on rows that tests/cpp/wide_visit_main.cpp dumped, for
// tests/test_gpu_wide_visit.py to compare with that program's words.
//   wide_visit_units <in.bin> <out.bin>
// in: 32 words per pair (node 20, origin 3, inverse direction 3, tmin, tmax, filter, padding 3);
// out: 8 words per pair (inner, leaf, nearest, t_rest bits: without, then with NAN_SAFE).
// Exit 2: bad arguments or files; exit 3: a HIP error (nothing is launched after one).
#include "sp_path.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace spd;
using namespace spm;

namespace {

constexpr int THREADS = 256;
constexpr int ROW = 32, OUT = 8;

#define HIP_OK(expr)                                                                                                   \
    do {                                                                                                               \
        const hipError_t e_ = (expr);                                                                                  \
        if (e_ != hipSuccess) {                                                                                        \
            std::fprintf(stderr, "wide_visit_units: %s: %s\n", #expr, hipGetErrorString(e_));                          \
            std::exit(3);                                                                                              \
        }                                                                                                              \
    } while (0)

template <bool NAN_SAFE>
__device__ __forceinline__ void one(const Scene& sc, uint32_t i, const uint32_t* r, uint32_t* o)
{
    Ray ray;
    ray.o = mk(__uint_as_float(r[0]), __uint_as_float(r[1]), __uint_as_float(r[2]));
    ray.d = mk(0.0f, 0.0f, 0.0f); // the visit reads the origin and the inverse direction only
    const f3       inv = mk(__uint_as_float(r[3]), __uint_as_float(r[4]), __uint_as_float(r[5]));
    const WideHits h   = wide_visit<NAN_SAFE>(sc, i, ray, inv, __uint_as_float(r[6]), __uint_as_float(r[7]), r[8]);
    o[0] = h.inner;
    o[1] = h.leaf;
    o[2] = (uint32_t)h.nearest;
    o[3] = __float_as_uint(h.t_rest);
}

// sc.wnodes: the pairs' node records, 5 x uint4 each; rays: 12 words per pair
__global__ __launch_bounds__(THREADS) void visit_kernel(Scene sc, const uint32_t* __restrict__ rays, uint32_t* __restrict__ out,
                                                        uint32_t n)
{
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    one<false>(sc, i, rays + 12 * (size_t)i, out + OUT * (size_t)i);
    one<true>(sc, i, rays + 12 * (size_t)i, out + OUT * (size_t)i + 4);
}

int fail(const char* msg)
{
    std::fprintf(stderr, "wide_visit_units: %s\n", msg);
    return 2;
}

} // namespace

int main(int argc, char** argv)
{
    if (argc != 3) return fail("usage: wide_visit_units <in.bin> <out.bin>");
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return fail("cannot open the input");
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    if (bytes <= 0 || bytes % (4 * ROW) != 0 || bytes / (4 * ROW) > (1l << 24)) { std::fclose(f); return fail("the input is no rows of 32 words"); }
    std::vector<uint32_t> in((size_t)bytes / 4);
    const size_t          got = std::fread(in.data(), 4, in.size(), f);
    std::fclose(f);
    if (got != in.size()) return fail("short read");
    const uint32_t        n = (uint32_t)(in.size() / ROW);
    std::vector<uint32_t> nodes((size_t)n * 20), rays((size_t)n * 12);
    for (uint32_t i = 0; i < n; ++i) {
        for (int j = 0; j < 20; ++j) nodes[(size_t)i * 20 + j] = in[(size_t)i * ROW + j];
        for (int j = 0; j < 12; ++j) rays[(size_t)i * 12 + j] = in[(size_t)i * ROW + 20 + j];
    }
    uint32_t *d_nodes = nullptr, *d_rays = nullptr, *d_out = nullptr;
    HIP_OK(hipMalloc(&d_nodes, nodes.size() * 4));
    HIP_OK(hipMalloc(&d_rays, rays.size() * 4));
    HIP_OK(hipMalloc(&d_out, (size_t)n * OUT * 4));
    HIP_OK(hipMemcpy(d_nodes, nodes.data(), nodes.size() * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_rays, rays.data(), rays.size() * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(d_out, 0xee, (size_t)n * OUT * 4));
    Scene sc = {};
    sc.wnodes = reinterpret_cast<const uint4*>(d_nodes);
    visit_kernel<<<(n + THREADS - 1) / THREADS, THREADS>>>(sc, d_rays, d_out, n);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    std::vector<uint32_t> out((size_t)n * OUT);
    HIP_OK(hipMemcpy(out.data(), d_out, out.size() * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipFree(d_nodes));
    HIP_OK(hipFree(d_rays));
    HIP_OK(hipFree(d_out));
    f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(out.data(), 4, out.size(), f) != out.size() || std::fclose(f) != 0) return fail("cannot write the output");
    std::printf("wide_visit %u\n", n);
    return 0;
}
