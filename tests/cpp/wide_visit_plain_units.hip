// wide_visit_plain_units.hip -- the plain node visit on the device (csrc/common/sp_wide_visit.h
// visit_plain; sp_path.hpp SP_VISIT_PLAIN), compiled with the library's numeric and device flags, for
// tests/test_gpu_wide_visit_plain.py.  Built twice (wide_visit_plain.mk): SP_VISIT_PLAIN=1, the
// library's default, and 0, the walks as they were before the plain form.
//   wide_visit_plain_units visits <in.bin> <out.bin>
//       in: 32 words per pair as tests/cpp/wide_visit_plain_main.cpp dumps them (node 20, origin 3,
//       inverse direction 3, tmin, tmax, filter, padding 3), every pair inside visit_plain's contract;
//       out: 4 words per pair (inner, leaf, nearest, t_rest bits) of spw::visit_plain -- with
//       SP_VISIT_PLAIN=0 of spw::visit<false>
//   wide_visit_plain_units walks <walk.bin> <out.bin>
//       walk.bin: that program's `walk` file (one tree, 256 rays = 4 waves); out: 3 words per ray --
//       wide_closest's primitive code and the bits of its t, wide_any's answer
// The merged-query walk of IterativeRRNEE (mq_run) is not reached from here: its queries are posted
// by integrate()'s own bookkeeping in LDS; the rrnee tests of the suite cover it.
// Exit 2: bad arguments or files; exit 3: a HIP error (nothing is launched after one).
#include "sp_path.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace spd;
using namespace spm;

namespace {

constexpr int THREADS = 256;
constexpr int ROW = 32, OUT = 4;
constexpr int STACK_DEPTH = 32; // entries per lane: 16 group entries and their 16 distances (wide_closest)

#define HIP_OK(expr)                                                                                                   \
    do {                                                                                                               \
        const hipError_t e_ = (expr);                                                                                  \
        if (e_ != hipSuccess) {                                                                                        \
            std::fprintf(stderr, "wide_visit_plain_units: %s: %s\n", #expr, hipGetErrorString(e_));                    \
            std::exit(3);                                                                                              \
        }                                                                                                              \
    } while (0)

// nodes: 20 words per pair; rays: 12 words per pair
__global__ __launch_bounds__(THREADS) void visit_kernel(const uint32_t* __restrict__ nodes, const uint32_t* __restrict__ rays,
                                                        uint32_t* __restrict__ out, uint32_t n)
{
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    uint32_t w[20];
    for (int j = 0; j < 20; ++j) w[j] = nodes[20 * (size_t)i + j];
    const uint32_t* r = rays + 12 * (size_t)i;
    const float     ox = __uint_as_float(r[0]), oy = __uint_as_float(r[1]), oz = __uint_as_float(r[2]);
    const float     ix = __uint_as_float(r[3]), iy = __uint_as_float(r[4]), iz = __uint_as_float(r[5]);
#if SP_VISIT_PLAIN
    const spw::Visit v = spw::visit_plain(w, ox, oy, oz, ix, iy, iz, __uint_as_float(r[6]), __uint_as_float(r[7]), r[8]);
#else
    const spw::Visit v = spw::visit<false>(w, ox, oy, oz, ix, iy, iz, __uint_as_float(r[6]), __uint_as_float(r[7]), r[8]);
#endif
    uint32_t* o = out + OUT * (size_t)i;
    o[0] = v.inner;
    o[1] = v.leaf;
    o[2] = (uint32_t)v.nearest;
    o[3] = __float_as_uint(v.t_rest);
}

// one block of four waves; rays: 8 floats each (o, tmin, d, tmax); out: 3 words per ray
__global__ __launch_bounds__(THREADS) void walk_kernel(Scene sc, const float* __restrict__ rays, uint32_t* __restrict__ out, uint32_t n)
{
    __shared__ uint32_t lds[(THREADS / 64) * STACK_DEPTH * 64];
    const uint32_t      i = threadIdx.x;
    if (i >= n) return;
    const Stack  st{ lds + (i >> 6) * STACK_DEPTH * 64, (int)(i & 63u), STACK_DEPTH };
    const float* q = rays + 8 * (size_t)i;
    Ray          ray;
    ray.o = mk(q[0], q[1], q[2]);
    ray.d = mk(q[4], q[5], q[6]);
    Hit h;
    h.t = q[7]; h.code = 0xffffffffu; h.beta = 0.0f; h.gamma = 0.0f; h.slot = 0xffffffffu;
    h = wide_closest<false>(sc, ray, q[3], h, st);
    const bool any = wide_any<false>(sc, ray, q[3], q[7], st);
    out[3 * i + 0] = h.code;
    out[3 * i + 1] = __float_as_uint(h.t);
    out[3 * i + 2] = any ? 1u : 0u;
}

int fail(const char* msg)
{
    std::fprintf(stderr, "wide_visit_plain_units: %s\n", msg);
    return 2;
}

bool read_words(const char* path, std::vector<uint32_t>& v)
{
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    if (bytes <= 0 || bytes % 4 != 0 || bytes > (1l << 30)) { std::fclose(f); return false; }
    v.resize((size_t)bytes / 4);
    const size_t got = std::fread(v.data(), 4, v.size(), f);
    std::fclose(f);
    return got == v.size();
}

bool write_words(const char* path, const std::vector<uint32_t>& v)
{
    FILE* f = std::fopen(path, "wb");
    return f && std::fwrite(v.data(), 4, v.size(), f) == v.size() && std::fclose(f) == 0;
}

uint32_t* to_device(const uint32_t* p, size_t words)
{
    uint32_t* d = nullptr;
    HIP_OK(hipMalloc(&d, words * 4));
    HIP_OK(hipMemcpy(d, p, words * 4, hipMemcpyHostToDevice));
    return d;
}

int visits(const std::vector<uint32_t>& in, const char* out_path)
{
    if (in.size() % ROW != 0 || in.size() / ROW > (1u << 24)) return fail("the input is no rows of 32 words");
    const uint32_t        n = (uint32_t)(in.size() / ROW);
    std::vector<uint32_t> nodes((size_t)n * 20), rays((size_t)n * 12);
    for (uint32_t i = 0; i < n; ++i) {
        for (int j = 0; j < 20; ++j) nodes[(size_t)i * 20 + j] = in[(size_t)i * ROW + j];
        for (int j = 0; j < 12; ++j) rays[(size_t)i * 12 + j] = in[(size_t)i * ROW + 20 + j];
    }
    uint32_t *d_nodes = to_device(nodes.data(), nodes.size()), *d_rays = to_device(rays.data(), rays.size()), *d_out = nullptr;
    HIP_OK(hipMalloc(&d_out, (size_t)n * OUT * 4));
    HIP_OK(hipMemset(d_out, 0xee, (size_t)n * OUT * 4));
    visit_kernel<<<(n + THREADS - 1) / THREADS, THREADS>>>(d_nodes, d_rays, d_out, n);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    std::vector<uint32_t> out((size_t)n * OUT);
    HIP_OK(hipMemcpy(out.data(), d_out, out.size() * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipFree(d_nodes));
    HIP_OK(hipFree(d_rays));
    HIP_OK(hipFree(d_out));
    if (!write_words(out_path, out)) return fail("cannot write the output");
    std::printf("visits %u plain %d\n", n, (int)SP_VISIT_PLAIN);
    return 0;
}

int walks(const std::vector<uint32_t>& in, const char* out_path)
{
    if (in.size() < 4) return fail("the walk file has no header");
    const size_t nrec = in[0], nslots = in[1], depth = in[2], nrays = in[3];
    if (nrec == 0 || nrec > (1u << 20) || nslots > (1u << 20) || nrays == 0 || nrays > (size_t)THREADS ||
        in.size() != 4 + 20 * nrec + 12 * nslots + 8 * nrays)
        return fail("the walk file's sizes do not add up");
    if (2 * (depth + 1) > (size_t)STACK_DEPTH) return fail("the tree is too deep for the unit's stack");
    // every child and leaf range the walks can reach stays inside the arrays
    for (size_t r = 0; r < nrec; ++r) {
        const uint32_t* w = &in[4 + 20 * r];
        for (int s = 0; s < 8; ++s) {
            const uint32_t meta = (w[6 + s / 4] >> (8 * (s % 4))) & 0xffu;
            if (((w[3] >> 24) >> s) & 1u) { if ((size_t)w[4] + (size_t)s >= nrec) return fail("a child leaves the records"); }
            else if (meta != 0u && (size_t)w[5] + (meta & 31u) + (meta >> 5) > nslots) return fail("a leaf range leaves the slots");
        }
    }
    uint32_t* d_nodes = to_device(&in[4], 20 * nrec);
    uint32_t* d_tris  = to_device(&in[4 + 20 * nrec], 12 * nslots);
    uint32_t* d_rays  = to_device(&in[4 + 20 * nrec + 12 * nslots], 8 * nrays);
    uint32_t* d_out   = nullptr;
    HIP_OK(hipMalloc(&d_out, nrays * 3 * 4));
    HIP_OK(hipMemset(d_out, 0xee, nrays * 3 * 4));
    Scene sc = {};
    sc.wnodes    = reinterpret_cast<const uint4*>(d_nodes);
    sc.wslot_tri = reinterpret_cast<const float4*>(d_tris);
    walk_kernel<<<1, THREADS>>>(sc, reinterpret_cast<const float*>(d_rays), d_out, (uint32_t)nrays);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    std::vector<uint32_t> out(nrays * 3);
    HIP_OK(hipMemcpy(out.data(), d_out, out.size() * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipFree(d_nodes));
    HIP_OK(hipFree(d_tris));
    HIP_OK(hipFree(d_rays));
    HIP_OK(hipFree(d_out));
    if (!write_words(out_path, out)) return fail("cannot write the output");
    std::printf("walks %zu plain %d\n", nrays, (int)SP_VISIT_PLAIN);
    return 0;
}

} // namespace

int main(int argc, char** argv)
{
    if (argc != 4) return fail("usage: wide_visit_plain_units visits|walks <in.bin> <out.bin>");
    std::vector<uint32_t> in;
    if (!read_words(argv[2], in)) return fail("cannot read the input");
    const std::string mode = argv[1];
    if (mode == "visits") return visits(in, argv[3]);
    if (mode == "walks") return walks(in, argv[3]);
    return fail("the mode is visits or walks");
}
