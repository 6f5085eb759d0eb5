// TEST PROGRAM: the denoiser's expressions (simplepath_amd/csrc/common/sp_denoise.h) on the host, in
// plain loops over a case file that tests/test_denoise_host.py writes.  What the device kernels do
// per lane -- prepare, the levels' taps through the inverse tile map, the finish -- is done here
// pixel by pixel with the same header, so its output must equal the numpy restatement
// (tests/_denoise.py) in every bit, and the tap count exactly.
//
//   denoise_host_main CASE OUT     prints "taps N"
//
// CASE (little endian): int32 width, height, slots, iterations, demodulate, has_albedo, has_normal,
// has_depth, has_coverage; float32 sigma_color, sigma_normal, sigma_depth, sigma_coverage,
// albedo_floor, depth_floor; int32 ids[slots]; then float32 colour [slots][64][3] and, where
// present, albedo [..][3], normal [..][3], depth [..], coverage [..].  OUT: float32 [slots][64][3].
#include "../../simplepath_amd/csrc/common/sp_denoise.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

template <typename T>
std::vector<T> read_n(FILE* f, size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "short case file\n");
        exit(2);
    }
    return v;
}

} // namespace

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<int32_t> hd = read_n<int32_t>(f, 9);
    const std::vector<float>   fl = read_n<float>(f, 6);
    const int    width = hd[0], height = hd[1], slots = hd[2], iterations = hd[3];
    const bool   demodulate = hd[4] != 0, has_a = hd[5] != 0, has_n = hd[6] != 0, has_z = hd[7] != 0, has_k = hd[8] != 0;
    const size_t px = (size_t)slots * 64;
    const std::vector<int32_t> ids      = read_n<int32_t>(f, (size_t)slots);
    const std::vector<float>   color    = read_n<float>(f, px * 3);
    const std::vector<float>   albedo   = read_n<float>(f, has_a ? px * 3 : 0);
    const std::vector<float>   normal   = read_n<float>(f, has_n ? px * 3 : 0);
    const std::vector<float>   depth    = read_n<float>(f, has_z ? px : 0);
    const std::vector<float>   coverage = read_n<float>(f, has_k ? px : 0);
    fclose(f);
    if (demodulate && !(has_a && has_k)) return 2;

    const float sigma_depth  = fl[2];
    const float albedo_floor = fl[4] == 0.0f ? spdn::k_albedo_floor : fl[4];
    const float depth_floor  = fl[5] == 0.0f ? spdn::k_depth_floor : fl[5];
    const int   tiles_x = (width + 7) / 8, tiles_y = (height + 7) / 8, total = tiles_x * tiles_y;

    // the inverse map: the lowest slot that lists a tile, -1: absent
    std::vector<int32_t> slot_of_tile((size_t)total, -1);
    for (int s = slots - 1; s >= 0; --s)
        if (ids[s] >= 0 && ids[s] < total) slot_of_tile[(size_t)ids[s]] = s;

    // every pixel slot's position, or x = -1 outside the image (and for an id outside the frame)
    std::vector<int> X(px, -1), Y(px, -1);
    for (int s = 0; s < slots; ++s) {
        if (ids[s] < 0 || ids[s] >= total) continue;
        for (int y = 0; y < 8; ++y)
            for (int x = 0; x < 8; ++x) {
                const int gx = (ids[s] % tiles_x) * 8 + x, gy = (ids[s] / tiles_x) * 8 + y;
                if (gx >= width || gy >= height) continue;
                const size_t i = (size_t)s * 64 + spdn::morton_lane((uint32_t)x, (uint32_t)y);
                X[i] = gx;
                Y[i] = gy;
            }
    }

    // prepare
    std::vector<spdn::Pixel> cur(px), next(px);
    for (size_t i = 0; i < px; ++i) {
        spdn::Pixel p{};
        if (X[i] >= 0) {
            if (has_n)
                for (int ch = 0; ch < 3; ++ch) p.n[ch] = normal[i * 3 + ch];
            if (has_k) p.k = coverage[i];
            if (has_z) p.z = depth[i];
            for (int ch = 0; ch < 3; ++ch) {
                p.x[ch] = color[i * 3 + ch];
                if (demodulate) p.x[ch] = p.x[ch] / spdn::albedo_scale(p.k, albedo[i * 3 + ch], albedo_floor);
            }
        }
        cur[i] = p;
    }

    // the levels
    unsigned long long taps = 0;
    for (int level = 0; level < iterations; ++level) {
        const spdn::Level L = spdn::level_constants(level, fl[0], fl[1], fl[3], has_n, has_k);
        for (size_t i = 0; i < px; ++i) {
            next[i] = cur[i];
            if (X[i] < 0) continue;
            const spdn::Pixel& c = cur[i];
            const float        g = has_z ? spdn::depth_gain(c.z, sigma_depth, depth_floor) : 0.0f;
            spdn::Accum        s;
            for (int dy = -2; dy <= 2; ++dy)
                for (int dx = -2; dx <= 2; ++dx) {
                    const int qx = X[i] + dx * L.step, qy = Y[i] + dy * L.step;
                    if (qx < 0 || qx >= width || qy < 0 || qy >= height) continue;
                    const int32_t sq = slot_of_tile[(size_t)((qy >> 3) * tiles_x + (qx >> 3))];
                    if (sq < 0) continue;
                    const spdn::Pixel& q = cur[(size_t)sq * 64 + spdn::morton_lane((uint32_t)qx, (uint32_t)qy)];
                    spdn::accumulate(s, spdn::tap_weight(q, c, g, L, spdn::spline(dx + 2) * spdn::spline(dy + 2)), q);
                }
            taps += s.taps;
            for (int ch = 0; ch < 3; ++ch) next[i].x[ch] = spdn::level_result(s, ch, c.x[ch]);
        }
        cur.swap(next);
    }

    // finish
    std::vector<float> out(px * 3, 0.0f);
    for (size_t i = 0; i < px; ++i) {
        if (X[i] < 0) continue;
        for (int ch = 0; ch < 3; ++ch)
            out[i * 3 + ch] = demodulate ? cur[i].x[ch] * spdn::albedo_scale(cur[i].k, albedo[i * 3 + ch], albedo_floor) : cur[i].x[ch];
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    if (!out.empty() && fwrite(out.data(), sizeof(float), out.size(), o) != out.size()) return 2;
    fclose(o);
    printf("taps %llu\n", taps);
    return 0;
}
