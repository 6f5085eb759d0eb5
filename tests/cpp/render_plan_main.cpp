// render_plan_main.cpp -- prints what simplepath_amd/csrc/hip/sp_plan.hpp decides for a table of
// requests (tests/test_render_plan.py holds the expected answers).  Plain C++17, no device:
//   g++ -std=c++17 -I <repo> tests/cpp/render_plan_main.cpp -o render_plan && ./render_plan
#include "simplepath_amd/csrc/hip/sp_plan.hpp"

#include <cstdio>
#include <vector>

using namespace splan;

static const char* name_of(int pipeline)
{
    switch (pipeline) {
    case SP_PIPELINE_WAVEFRONT: return "wavefront";
    case SP_PIPELINE_MEGAKERNEL: return "megakernel";
    case SP_PIPELINE_SAMPLE_CHUNKS: return "chunks";
    default: return "auto";
    }
}

static void plan_row(const char* label, PlanIn in, const RenderHooks& hooks = RenderHooks{})
{
    const Plan pl = plan_render(in, hooks);
    std::printf("plan %s %s %d\n", label, name_of(pl.pipeline), pl.tail_auto ? 1 : 0);
}

int main()
{
    // an MI355X: 256 CUs, 4096 persistent waves at full occupancy; a budget every case below fits
    PlanIn base;
    base.integ     = SP_INTEGRATOR_DIRECT_LIGHTING;
    base.spp       = 256;
    base.n_lights  = 1; // bunny.sp: 30 generations per pixel at 256 spp
    base.n_cu      = 256;
    base.ck_budget = 96e9;
    auto with = [&](int64_t tiles, uint32_t spp, bool image_light = false) {
        PlanIn in      = base;
        in.n_tiles     = tiles;
        in.spp         = spp;
        in.image_light = image_light;
        return in;
    };
    plan_row("frame_1080p", with(32400, 256));
    plan_row("shard_2way", with(16200, 256));
    plan_row("shard_4way", with(8100, 256));
    plan_row("shard_8way", with(4050, 256));
    {
        PlanIn in    = with(8100, 256);
        in.ck_budget = (double)chunk_plan(8100, 256, 0, 1, false, RenderHooks{}).total - 1.0;
        plan_row("shard_4way_over_budget", in);
    }
    plan_row("image_light_16384_64spp", with(16384, 64, true));
    plan_row("image_light_16383_64spp", with(16383, 64, true));
    plan_row("image_light_8100", with(8100, 256, true));
    plan_row("shard_2way_127spp", with(16200, 127));
    {
        PlanIn in        = with(16200, 256);
        in.tail_fraction = -1.0f;
        plan_row("shard_2way_tail_off", in);
    }
    for (int64_t tiles : { 64, 8100, 32400, 200000 }) {
        PlanIn in = with(tiles, 256);
        in.integ  = SP_INTEGRATOR_ITERATIVE_RRNEE;
        char label[32];
        std::snprintf(label, sizeof(label), "rrnee_%lld", (long long)tiles);
        plan_row(label, in);
    }
    {
        PlanIn in   = with(32400, 256);
        in.n_lights = 1001;
        plan_row("lights_1001", in);
        in.n_lights = 1000;
        plan_row("lights_1000", in);
    }
    {
        RenderHooks hooks;
        hooks.wave_min_tiles = 8100;
        plan_row("wave_hook_at", with(8100, 256), hooks);
        plan_row("wave_hook_below", with(8099, 256), hooks);
        PlanIn in   = with(8100, 256);
        in.n_lights = 33; // above the wavefront's light mask
        plan_row("wave_hook_33_lights", in, hooks);
        in       = with(8100, 256);
        in.integ = SP_INTEGRATOR_WHITTED;
        plan_row("wave_hook_whitted", in, hooks);
    }
    {
        PlanIn in = with(32400, 256); // a pipeline asked for by name is kept
        in.asked  = SP_PIPELINE_SAMPLE_CHUNKS;
        plan_row("asked_chunks", in);
        in.asked = SP_PIPELINE_WAVEFRONT;
        plan_row("asked_wavefront", in);
    }

    auto chunk_row = [](const char* label, int64_t tiles, uint32_t spp, int64_t req) {
        const ChunkPlan c = chunk_plan(tiles, spp, req, 2, false, RenderHooks{});
        std::printf("chunks %s %lld %u\n", label, (long long)c.chunks, c.len);
    };
    chunk_row("auto_4050", 4050, 256, 0);
    chunk_row("req_3_of_5", 1000, 5, 3);
    chunk_row("req_above_spp", 1000, 5, 9);
    {
        RenderHooks replay;
        replay.chunk_replay = true;
        std::printf("draws plain %d\n", chunk_plan(100, 4, 0, 2, false, RenderHooks{}).known_draws ? 1 : 0);
        std::printf("draws image_light %d\n", chunk_plan(100, 4, 0, 2, true, RenderHooks{}).known_draws ? 1 : 0);
        std::printf("draws lights_1001 %d\n", chunk_plan(100, 4, 0, 1001, false, RenderHooks{}).known_draws ? 1 : 0);
        std::printf("draws replay_hook %d\n", chunk_plan(100, 4, 0, 2, false, replay).known_draws ? 1 : 0);
    }

    const int32_t tiles_x = 240; // 1920 / 8
    auto stride = [](int32_t first, int32_t k, int n) {
        std::vector<int32_t> v;
        for (int i = 0; i < n; ++i) v.push_back(first + i * k);
        return v;
    };
    std::printf("neighbours frame %d\n", order_neighbours(nullptr, false, 32400, tiles_x));
    std::printf("neighbours device_list %d\n", order_neighbours(nullptr, true, 100, tiles_x));
    for (int k : { 1, 2, 8, 7 }) {
        const std::vector<int32_t> v = stride(k == 7 ? 3 : 0, k, 1000);
        std::printf("neighbours stride_%d %d\n", k, order_neighbours(v.data(), true, (int64_t)v.size(), tiles_x));
    }
    {
        std::vector<int32_t> v = stride(0, 2, 1000);
        v[500] += 1;
        std::printf("neighbours irregular %d\n", order_neighbours(v.data(), true, (int64_t)v.size(), tiles_x));
        std::printf("neighbours one_tile %d\n", order_neighbours(v.data(), true, 1, tiles_x));
        std::vector<int32_t> down = stride(5000, -2, 100);
        std::printf("neighbours descending %d\n", order_neighbours(down.data(), true, (int64_t)down.size(), tiles_x));
    }
    return 0;
}
