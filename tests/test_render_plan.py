"""How a render request is carried out, decided without a device: the AUTO pipeline choice, the
tail-chunk rule, the sample-chunk plan and the tile order's queue neighbours of
simplepath_amd/csrc/hip/sp_plan.hpp, printed by tests/cpp/render_plan_main.cpp (plain g++) for a
table of requests.  The expected answers follow from the measured configurations the rule's
comments name (DESIGN.md sections 3, 6, 12): an MI355X has 256 CUs, so 4096 persistent waves."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PLANS = {
    # label: (pipeline, tail chunks wanted)
    "frame_1080p": ("megakernel", 1),              # 2 x 32400 >= 5 x 4096
    "shard_2way": ("megakernel", 1),               # 32400 >= 20480
    "shard_4way": ("chunks", 0),                   # 16200 < 20480; below 24000 tiles
    "shard_8way": ("chunks", 0),
    "shard_4way_over_budget": ("megakernel", 0),   # the chunk buffers one byte over the budget
    "image_light_16384_64spp": ("megakernel", 1),  # 16384 >= 4 x 4096 from 64 spp
    "image_light_16383_64spp": ("megakernel", 0),  # 16383 >= 24000 / 2: no chunks; below the tail bound
    "image_light_8100": ("chunks", 0),             # 8100 < 12000
    "shard_2way_127spp": ("chunks", 0),            # below 128 spp
    "shard_2way_tail_off": ("chunks", 0),          # tail_fraction < 0
    "rrnee_64": ("megakernel", 0),
    "rrnee_8100": ("megakernel", 0),
    "rrnee_32400": ("megakernel", 0),
    "rrnee_200000": ("megakernel", 0),
    "lights_1001": ("megakernel", 0),              # draw counts not known from the camera hits
    "lights_1000": ("megakernel", 1),
    "wave_hook_at": ("wavefront", 0),              # SP_WAVE_MIN_TILES at the tile count
    "wave_hook_below": ("chunks", 0),
    "wave_hook_33_lights": ("megakernel", 0),      # no wavefront above 32 lights; 923 generations per pixel: over budget
    "wave_hook_whitted": ("megakernel", 0),
    "asked_chunks": ("chunks", 1),                 # a pipeline asked for by name is kept
    "asked_wavefront": ("wavefront", 1),
}
CHUNKS = {"auto_4050": (32, 8), "req_3_of_5": (3, 2), "req_above_spp": (5, 1)}
DRAWS = {"plain": 1, "image_light": 0, "lights_1001": 0, "replay_hook": 0}
NEIGHBOURS = {
    "frame": 240,        # a whole frame: the tile below is tiles_x entries on
    "device_list": 0,    # the host does not know the list
    "stride_1": 240,
    "stride_2": 120,     # k divides tiles_x: tiles_x / k
    "stride_8": 30,
    "stride_7": -1,      # k does not divide 240: the +-1 entries only
    "irregular": 0,
    "one_tile": 0,
    "descending": 0,
}


@pytest.fixture(scope="module")
def decisions(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("render_plan") / "render_plan")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", ROOT,
                    os.path.join(ROOT, "tests", "cpp", "render_plan_main.cpp"), "-o", exe], check=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout
    rows = {}
    for line in out.splitlines():
        kind, label, *values = line.split()
        rows.setdefault(kind, {})[label] = values
    return rows


def test_auto_pipeline_and_tail_rule(decisions):
    got = {k: (v[0], int(v[1])) for k, v in decisions["plan"].items()}
    assert got == PLANS


def test_chunk_plan(decisions):
    assert {k: (int(v[0]), int(v[1])) for k, v in decisions["chunks"].items()} == CHUNKS
    assert {k: int(v[0]) for k, v in decisions["draws"].items()} == DRAWS


def test_order_neighbours(decisions):
    assert {k: int(v[0]) for k, v in decisions["neighbours"].items()} == NEIGHBOURS
