// sp_plan.hpp -- how a render request is carried out, decided from plain numbers: the environment
// test hooks of the render path, the sample-chunk buffer plan, the tile order's queue neighbours,
// the tail-chunk rule and the AUTO pipeline choice.  No HIP in here: sp_capi.hip applies the
// decisions, and tests/cpp/render_plan_main.cpp checks them without a device.
#pragma once

#include "../../../include/simplepath_hip.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>

// Megakernel tail chunks: the fraction of the tiles cut into sample chunks at the end of the queue,
// and chunks per tile.
#ifndef SP_TAIL_FRAC
#define SP_TAIL_FRAC 0.12f
#endif
#ifndef SP_TAIL_CHUNKS
#define SP_TAIL_CHUNKS 64
#endif
// The sample-chunk pipeline's fused form: on, and the preps placed ahead of the first chunks =
// persistent waves / SP_CK_FRONT_DIV
#ifndef SP_CK_FUSED
#define SP_CK_FUSED 1
#endif
#ifndef SP_CK_CAMFOLD
#define SP_CK_CAMFOLD 1
#endif
#ifndef SP_CK_CAM_BLOCK
#define SP_CK_CAM_BLOCK 32
#endif
#ifndef SP_CK_FRONT_DIV
#define SP_CK_FRONT_DIV 8
#endif
#ifndef SP_TILE_STRIDE_ROW
#define SP_TILE_STRIDE_ROW 1
#endif

namespace splan {

// sp_capi.hip asserts these against their owners (sp_rng.h, sp_device.hpp, sp_wave.hpp)
constexpr int MT_N          = 312;
constexpr int MT_GEN_WORDS  = MT_N * 64; // words of one generation buffer of a wave slot
constexpr int WF_MAX_LIGHTS = 32;

// The environment test hooks of the render path, read once at the top of every call (the tests set
// them with monkeypatch between calls).  An explicit sp_render_params field wins over its hook, the
// hook over the compiled default held here.
struct RenderHooks {
    int64_t     wave_min_tiles  = INT64_MAX;       // SP_WAVE_MIN_TILES: AUTO takes the wavefront from here
    int64_t     chunk_max_tiles = 24000;           // SP_CHUNK_MAX_TILES: AUTO takes the sample chunks below
    int64_t     chunks          = 0;               // SP_CHUNKS: chunks per pixel (0: automatic)
    double      chunk_max_gb    = 96.0;            // SP_CHUNK_MAX_GB: budget of the chunk and tail buffers
    bool        chunk_replay    = false;           // SP_CHUNK_REPLAY: draw counts replayed on the stream
    double      wave_max_gb     = 64.0;            // SP_WAVE_MAX_GB: wavefront state per pass (of 288 GB HBM)
    const char* wave_diag       = nullptr;         // SP_WAVE_DIAG=<file>
    bool        ck_fused        = SP_CK_FUSED != 0;
    bool        ck_camfold      = SP_CK_CAMFOLD != 0;
    uint32_t    ck_cam_block    = SP_CK_CAM_BLOCK;
    int         ck_front_div    = SP_CK_FRONT_DIV;
    const char* tile_diag       = nullptr;         // SP_TILE_DIAG=<file>
    int         probe_step      = 0;               // SP_PROBE_STEP (0: automatic)
    bool        tail_frac_set   = false;           // SP_TAIL_FRAC (A/B runs; 0: off)
    float       tail_frac       = 0.0f;
    int         tail_chunks     = SP_TAIL_CHUNKS;

    static RenderHooks from_env()
    {
        RenderHooks h;
        if (const char* v = std::getenv("SP_WAVE_MIN_TILES")) h.wave_min_tiles = std::atoll(v);
        if (const char* v = std::getenv("SP_CHUNK_MAX_TILES")) h.chunk_max_tiles = std::atoll(v);
        if (const char* v = std::getenv("SP_CHUNKS")) h.chunks = std::max<int64_t>(1, std::atoll(v));
        if (const char* v = std::getenv("SP_CHUNK_MAX_GB")) h.chunk_max_gb = std::atof(v);
        if (const char* v = std::getenv("SP_CHUNK_REPLAY")) h.chunk_replay = std::atoi(v) != 0;
        if (const char* v = std::getenv("SP_WAVE_MAX_GB")) h.wave_max_gb = std::atof(v);
        h.wave_diag = std::getenv("SP_WAVE_DIAG");
        if (const char* v = std::getenv("SP_CK_FUSED")) h.ck_fused = std::atoi(v) != 0;
        if (const char* v = std::getenv("SP_CK_CAMFOLD")) h.ck_camfold = std::atoi(v) != 0;
        if (const char* v = std::getenv("SP_CK_CAM_BLOCK")) h.ck_cam_block = (uint32_t)std::max(1, std::atoi(v));
        if (const char* v = std::getenv("SP_CK_FRONT_DIV")) h.ck_front_div = std::max(1, std::atoi(v));
        h.tile_diag = std::getenv("SP_TILE_DIAG");
        if (const char* v = std::getenv("SP_PROBE_STEP")) h.probe_step = std::max(1, std::atoi(v));
        if (const char* v = std::getenv("SP_TAIL_FRAC")) {
            h.tail_frac_set = true;
            h.tail_frac     = (float)std::atof(v);
        }
        if (const char* v = std::getenv("SP_TAIL_CHUNKS")) h.tail_chunks = std::atoi(v);
        return h;
    }
};

// Sample-chunk buffer plan (sp_chunk.hip): the same sizes decide AUTO and are allocated.
struct ChunkPlan {
    int64_t  chunks = 1;    // chunks per pixel
    uint32_t len = 1;       // samples per chunk (the last may be short)
    uint32_t gens = 0;      // generator-store generations per pixel
    bool     known_draws = true;
    size_t   b_hits = 0, b_L = 0, b_snap = 0, b_ctl = 0, b_draws = 0, total = 0;
};
inline ChunkPlan chunk_plan(int64_t n_tiles, uint32_t spp, int64_t chunks_req, int n_lights, bool image_light,
                            const RenderHooks& hooks)
{
    ChunkPlan c;
    // chunks per pixel: the smallest power of two (<= 32) giving ~120K (tile, chunk) items (the
    // best of the bunny 2/4/8-way shard sweep) unless the caller asks for a count
    c.chunks = 1;
    while (c.chunks < 32 && n_tiles * c.chunks < 120000) c.chunks *= 2;
    if (chunks_req > 0) c.chunks = chunks_req;
    c.chunks = std::min<int64_t>(c.chunks, spp);
    c.len    = (uint32_t)((spp + c.chunks - 1) / c.chunks);
    c.chunks = (spp + c.len - 1) / c.len;
    // a DirectLighting sample draws at most 34 words per light (Light::sample 2 + glossy rho 32);
    // +2 generations for the first twist and the one rng_prepare may twist ahead
    const uint64_t max_draws = (uint64_t)spp * (uint64_t)std::max(1, n_lights) * 34;
    c.gens = (uint32_t)((max_draws + MT_N - 1) / MT_N + 2);
    // per-sample draw counts from the camera pass unless an image light makes them depend on the
    // drawn numbers (then ck_count replays Light::sample); SP_CHUNK_REPLAY=1 forces the replay (test)
    c.known_draws = n_lights <= 1000 && !image_light && !hooks.chunk_replay;
    const size_t n_px = (size_t)n_tiles * 64;
    c.b_hits  = n_px * spp * 16;
    c.b_L     = n_px * spp * 12;
    c.b_snap  = (size_t)n_tiles * c.gens * MT_GEN_WORDS * 8;
    c.b_ctl   = (size_t)c.chunks * n_px * 4;
    c.b_draws = c.known_draws ? n_px * spp * 2 : 0;
    c.total   = c.b_hits + c.b_L + c.b_snap + c.b_ctl + c.b_draws + 4 * 256;
    return c;
}

// Queue neighbours of the tile-order kernel's cost estimate (sp_mega.hip tile_est): > 0 the queue
// offset of the tile below, -1 the +-1 queue neighbours only, 0 none.  The tile ids are row-major
// (base/TileScheduler.h:75-77: x = index % tiles_x), so for a whole frame (k = 1) the +-1 queue
// neighbours are the tiles left and right.  For a host list with a constant stride k > 1 (a rank's
// interleaved shard) they are the tiles k columns to the left and right -- the same row, not
// adjacent -- and the tile below is tiles_x / k entries on when k divides tiles_x; otherwise
// (-1) the rows of consecutive entries shift and only the +-1 entries are used.  SP_TILE_STRIDE_ROW
// 0 drops the +-1 entries for k > 1 (the column blend alone, or the probe time alone when k does
// not divide tiles_x).  Row blend kept for k > 1 by an A/B on elf's 8-way shard.
// host_ids: the list where the host has it (nullptr with `listed`: a device list, no neighbours).
inline int order_neighbours(const int32_t* host_ids, bool listed, int64_t n_tiles, int32_t tiles_x)
{
    if (!listed) return tiles_x;
    if (!host_ids || n_tiles < 2) return 0;
    const int64_t k = (int64_t)host_ids[1] - host_ids[0];
    if (k <= 0) return 0;
    for (int64_t i = 2; i < n_tiles; ++i)
        if ((int64_t)host_ids[i] - host_ids[i - 1] != k) return 0;
    if (k > 1 && !SP_TILE_STRIDE_ROW) return (tiles_x % k == 0) ? -(int)(tiles_x / k) - 1 : 0;
    return (tiles_x % k == 0) ? (int)(tiles_x / k) : -1;
}

// Megakernel tail chunks (sp_capi.hip mega_plan_tail): DirectLighting from 2.5 tiles per persistent
// wave (16 per CU at full occupancy) and 128 spp, where the draw counts are known from the camera
// hits.  There the megakernel with its tile order and tail chunks beats the sample chunks (bunny
// 2-way shard 16200 tiles: 3620-3640 against 3170 Mrays/s, lucy 2-way 3227 against 2885; 3-way, 2.6
// tiles per wave: 3398-3412 at a fraction of 0.4 against the fused chunks' 3321-3344; 4-way, 2 per
// wave: 2820-2980 against 3297 -- profiles/r06/tail/ab_shards*.log, ab_fused*.log).
// With an image light the preps replay Light::sample (TailArgs::replay): material_spheres with its
// image light, 1024^2 @ 64 spp (4 tiles per wave), 3814-3826 -> 3890-3895 Mrays/s (ab_spheres.log),
// so from 64 spp at 4 tiles per wave as well.
inline bool tail_auto(int32_t integ, int64_t n_tiles, uint32_t spp, int n_lights, int n_cu, float tail_fraction)
{
    const int64_t tail_waves = (int64_t)std::max(1, n_cu) * 16;
    return integ == SP_INTEGRATOR_DIRECT_LIGHTING && n_lights <= 1000 && tail_fraction >= 0.0f &&
           ((spp >= 128 && 2 * n_tiles >= 5 * tail_waves) || (spp >= 64 && n_tiles >= 4 * tail_waves));
}

// the wavefront pipeline implements DirectLighting with a light mask of one u32 per pixel
inline bool wave_ok(int32_t integ, int n_lights) { return integ == SP_INTEGRATOR_DIRECT_LIGHTING && n_lights <= WF_MAX_LIGHTS; }

struct PlanIn {
    int32_t  integ       = SP_INTEGRATOR_DIRECT_LIGHTING; // resolved
    int64_t  n_tiles     = 0;
    uint32_t spp         = 1;
    int      n_lights    = 0;
    bool     image_light = false;
    int      n_cu        = 0;
    float    tail_fraction = 0.0f; // sp_render_params
    int64_t  chunks_req  = 0;      // sp_render_params.chunks_per_pixel
    double   ck_budget   = 0.0;    // bytes the sample-chunk buffers may take
    int      asked       = SP_PIPELINE_AUTO; // the pipeline asked for by name, or AUTO
};
struct Plan {
    int       pipeline  = SP_PIPELINE_MEGAKERNEL;
    bool      tail_auto = false;
    ChunkPlan cp;
};

// AUTO (measurements: DESIGN.md §3, §6).  The megakernel renders the 1-GPU frame fastest
// (bunny 1080p @ 256 spp: 2974 Mrays/s, wavefront 2305).  Below SP_CHUNK_MAX_TILES = 24000
// tiles (the 2-8-GPU shards) one pixel's sample chain bounds the megakernel and the sample
// chunks win (8-way shard 2444 against 823), when their buffers fit the budget.  With an image
// light ck_count replays Light::sample, so the chunks pay off only below half that (spheres
// 1024^2 @ 64 spp, 16384 tiles: chunks 2902, megakernel 2973).  The wavefront runs on request,
// or from SP_WAVE_MIN_TILES tiles (test hook).  A pipeline asked for by name is kept.
inline Plan plan_render(const PlanIn& in, const RenderHooks& hooks)
{
    Plan pl;
    const int64_t chunks_req = in.chunks_req ? in.chunks_req : hooks.chunks;
    pl.cp        = chunk_plan(in.n_tiles, in.spp, chunks_req, in.n_lights, in.image_light, hooks);
    pl.tail_auto = tail_auto(in.integ, in.n_tiles, in.spp, in.n_lights, in.n_cu, in.tail_fraction);
    pl.pipeline  = in.asked;
    if (in.asked == SP_PIPELINE_AUTO) {
        const int64_t chunk_max = in.image_light ? hooks.chunk_max_tiles / 2 : hooks.chunk_max_tiles;
        if (wave_ok(in.integ, in.n_lights) && in.n_tiles >= hooks.wave_min_tiles) pl.pipeline = SP_PIPELINE_WAVEFRONT;
        else if (pl.tail_auto) pl.pipeline = SP_PIPELINE_MEGAKERNEL;
        else if (in.integ == SP_INTEGRATOR_DIRECT_LIGHTING && in.n_tiles < chunk_max && (double)pl.cp.total <= in.ck_budget)
            pl.pipeline = SP_PIPELINE_SAMPLE_CHUNKS;
        else pl.pipeline = SP_PIPELINE_MEGAKERNEL; // also when the chunk buffers would not fit the budget
    }
    return pl;
}

} // namespace splan
