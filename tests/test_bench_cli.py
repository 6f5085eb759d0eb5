"""bench.py's plain run and its options: a plain run prints the line without the CPU baseline and
parity objects (those are --full's), --steps sets the number of timed frames, and --dump-outputs
writes the last timed frame -- the same bytes from run to run, and the frame the render call
computes.  On CPU the SP_BENCH_CPU_RENDER hook renders with the oracle; on the GPU the dump is
compared with the same render made in this process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import simplepath_amd as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP = 40, 24, 2  # 15 tiles of 8x8


def run_bench(out_dir, *extra, env=None):
    e = dict(os.environ, **(env or {}))
    e.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--width", str(W), "--height", str(H), "--spp", str(SPP), "--dump-outputs", str(out_dir),
                        *extra], capture_output=True, text=True, timeout=240, env=e, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    tiles = np.load(os.path.join(out_dir, "radiance_tiles.npy"))
    stats = np.load(os.path.join(out_dir, "render_stats.npy"))
    return line, tiles, stats


def check_line_and_dump(line, tiles, stats):
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["unit"] == "Mrays/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["cpu_baseline"] is None and line["parity"] is None  # --full's
    assert tiles.dtype == np.float32 and tiles.shape == (line["config"]["tiles"], 64, 3) == (15, 64, 3)
    assert stats.dtype == np.float64 and stats[0] == line["rays_per_step"] and stats[2] == W * H * SPP


def test_plain_run_dumps_the_frame(tmp_path):
    from tests import _oracle

    env = {"SP_BENCH_CPU_RENDER": "1", "OMP_NUM_THREADS": "2"}
    line, tiles, stats = run_bench(tmp_path / "a", env=env)
    check_line_and_dump(line, tiles, stats)
    s = sp.Scene.from_file(_scene_path())
    s.set_resolution(W, H)
    ref, st = _oracle.render(s, sp.string_to_integrator_type("direct_lighting"), SPP, None, threads=2, variant="glibc")
    assert np.array_equal(tiles.view(np.uint32), ref.view(np.uint32))
    assert stats[0] == st["rays"] and stats[1] == st["shadow_rays"]


def test_dump_is_capped_with_a_fixed_sample(tmp_path, monkeypatch):
    import importlib.util

    import torch
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    monkeypatch.setattr(b, "DUMP_MAX_BYTES", 10 * 64 * 3 * 4)
    t = torch.arange(25 * 64 * 3, dtype=torch.float32).reshape(25, 64, 3)

    class St:
        rays, shadow_rays, samples, rng_draws = 7, 3, 4, 9
    b.dump_outputs(str(tmp_path / "a"), t, St)
    b.dump_outputs(str(tmp_path / "b"), t, St)
    a = np.load(tmp_path / "a" / "radiance_tiles.npy")
    assert a.shape == (10, 64, 3) and a.nbytes <= b.DUMP_MAX_BYTES
    assert np.array_equal(a, np.load(tmp_path / "b" / "radiance_tiles.npy"))
    rows = (a[:, 0, 0] / (64 * 3)).astype(int)
    assert np.all(np.diff(rows) > 0) and np.array_equal(a, t.numpy()[rows])  # whole tiles, ascending
    assert np.array_equal(np.load(tmp_path / "a" / "render_stats.npy"), [7.0, 3.0, 4.0, 9.0])


@pytest.mark.gpu
def test_plain_run_dumps_the_frame_gpu(tmp_path):
    line, tiles, stats = run_bench(tmp_path / "a")
    check_line_and_dump(line, tiles, stats)
    assert line["roofline"] is not None and line["library"] is not None
    s = sp.Scene.from_file(_scene_path())
    s.set_resolution(W, H)
    s.upload(device=0, bvh_mode=0)
    ids = np.arange(sp.ColumnMajorTileScheduler(W, H).get_num_tiles(), dtype=np.int32)
    mine, st = sp.render_tiles(s, "direct_lighting", SPP, ids)
    assert np.array_equal(tiles.view(np.uint32), mine.view(np.uint32))
    assert stats[0] == st.rays and stats[3] == st.rng_draws


def _scene_path():
    """The scene file the benchmark renders: written once into its scene directory, by it or here."""
    import tempfile

    from simplepath_amd import scenes
    return scenes.write_bunny_scene(os.path.join(tempfile.gettempdir(), f"sp_bench_{os.getuid()}"))
