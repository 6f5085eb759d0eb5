"""Progressive renders on the device (sp_progress, include/simplepath_hip.h): k passes of samples
give the bits of one pass, which the parity suite pins to the CPU oracle and the reference build.

What is carried between passes is each pixel's std::mt19937_64 position, its undivided sum and the
sample count; the corners are the generation boundaries of the stream (a pass ending on word 312 of
a generation, or right after the seed's first twist), data-dependent draw counts (an image light),
IterativeRRNEE's estimates served across lanes, clipped border tiles and tile lists with their own
slots, and the checkpoint (export / import) through the documented host format."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import simplepath_amd as sp
from simplepath_amd import _abi
from tests import _oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_INTEGRATORS = ["mandelbrot", "brute_force", "brute_force_iterative", "brute_force_iterative_rr", "iterative_rrnee",
                   "direct_lighting", "whitted"]


def load(scene_dir, name, w, h, bvh=0):
    s = sp.Scene.from_file(os.path.join(scene_dir, name))
    s.set_resolution(w, h)
    s.upload(device=0, bvh_mode=bvh)
    return s


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def counts(st):
    return (st.rays, st.shadow_rays, st.samples, st.rng_draws)


def run_passes(prog, passes):
    """Render the passes; returns (last image, per-field sums of the calls' stats)."""
    total = np.zeros(4, dtype=np.int64)
    img = None
    for k in passes:
        img, st = prog.render(k)
        assert st.samples > 0 or img.size == 0
        total += np.array(counts(st), dtype=np.int64)
    return img, tuple(int(x) for x in total)


def one_shot(s, integrator, spp, ids=None, **kw):
    return sp.render_tiles(s, integrator, spp, ids, pipeline="megakernel", tail_fraction=-1.0, **kw)


def pixel_xy(w, tile, m):
    """image pixel of morton index m of a tile (lane = pixel, sp_tiles_to_image's order)"""
    dx = (m & 1) | ((m >> 1) & 2) | ((m >> 2) & 4)
    dy = ((m >> 1) & 1) | ((m >> 2) & 2) | ((m >> 3) & 4)
    tw = (w + 7) // 8
    return (tile % tw) * 8 + dx, (tile // tw) * 8 + dy


# ---- 1. oracle parity across generation boundaries ------------------------------------------

def test_passes_match_the_oracle_at_every_stop(scene_dir):
    # a glossy pixel draws ~34 words per sample: over 40 samples the streams cross three or four
    # 312-word generations, and the passes end at varied positions in them
    s = load(scene_dir, "bunny.sp", 64, 40, bvh=1)
    integ = sp.string_to_integrator_type("direct_lighting")
    prog = sp.Progressive(s, "direct_lighting")
    rays = shadow = done = 0
    for k in (1, 2, 5, 13, 19):
        img, st = prog.render(k)
        done += k
        rays += st.rays
        shadow += st.shadow_rays
        assert prog.samples == done
        ref, rst = _oracle.render(s, integ, done, variant="spm")
        assert same_bits(img, ref), done
    assert done == 40 and (rays, shadow) == (rst["rays"], rst["shadow_rays"])
    prog.close()


# ---- 2. passes equal one shot, every integrator -----------------------------------------------

@pytest.mark.parametrize("bvh", [0, 1])
@pytest.mark.parametrize("scene_name", ["closed_room.sp", "elf_small.sp"])
@pytest.mark.parametrize("integrator", ALL_INTEGRATORS)
def test_passes_equal_one_shot(scene_dir, integrator, scene_name, bvh):
    s = load(scene_dir, scene_name, 40, 24, bvh=bvh)
    ref, rst = one_shot(s, integrator, 8)
    for passes in ((1, 3, 4), (1,) * 8):
        with sp.Progressive(s, integrator) as prog:
            img, total = run_passes(prog, passes)
            assert prog.samples == 8
        assert same_bits(img, ref), passes
        assert total == counts(rst), passes


@pytest.mark.parametrize("waves", [2, 4])
def test_rrnee_occupancy_variants(scene_dir, waves):
    s = load(scene_dir, "elf_small.sp", 40, 24)
    ref, rst = one_shot(s, "iterative_rrnee", 8)
    with sp.Progressive(s, "iterative_rrnee", waves_per_simd=waves) as prog:
        img, total = run_passes(prog, (1, 3, 4))
    assert same_bits(img, ref) and total == counts(rst)


# ---- 3. image light: data-dependent draw counts -----------------------------------------------

@pytest.mark.parametrize("bvh", [0, 1])
@pytest.mark.parametrize("integrator", ["direct_lighting", "iterative_rrnee"])
def test_image_light(scene_dir, integrator, bvh):
    s = load(scene_dir, "material_spheres_ibl.sp", 48, 32, bvh=bvh)
    ref, rst = one_shot(s, integrator, 5)
    with sp.Progressive(s, integrator) as prog:
        img, total = run_passes(prog, (2, 3))
    assert same_bits(img, ref) and total == counts(rst)


# ---- 4. long chain ----------------------------------------------------------------------------

@pytest.mark.parametrize("integrator", ["direct_lighting", "iterative_rrnee"])
def test_long_chain(scene_dir, integrator):
    # the glossy-heavy tile of test_gpu_edges.py::test_long_sample_chain: ~40 generations per pixel
    s = load(scene_dir, "bunny.sp", 16, 8, bvh=1)
    ids = np.array([0], dtype=np.int32)
    ref, rst = one_shot(s, integrator, 600, ids)
    with sp.Progressive(s, integrator, ids) as prog:
        img, total = run_passes(prog, (7, 293, 300))
        state, n = prog.export_state()
    assert n == 600 and same_bits(img, ref) and total == counts(rst)
    assert int(state["draws"].max()) > 312 * 30
    assert int(state["draws"].sum()) == rst.rng_draws


def test_pass_ending_on_a_generations_last_word(scene_dir):
    # material_spheres.sp has two lights (environment + sphere): a DirectLighting sample on a
    # Lambertian surface draws Light::sample's two words per light and nothing else, 4 words, so after
    # 78 samples such a pixel has drawn exactly 312: the pass ends on the last word of generation 1,
    # in mid-stream.  The next draw must come from generation 2, whether or not it was twisted ahead.
    s = load(scene_dir, "material_spheres.sp", 24, 48, bvh=1)
    ref, rst = one_shot(s, "direct_lighting", 156)
    with sp.Progressive(s, "direct_lighting") as prog:
        _, st1 = prog.render(78)
        state, _ = prog.export_state()
        on_edge = state["draws"] == 312
        print(f"{int(on_edge.sum())} pixels ended the pass on word 312; their mt_pos: {sorted(set(state['mt_pos'][on_edge].tolist()))}")
        assert on_edge.any() and np.isin(state["mt_pos"][on_edge], (0, 312)).all()
        _, st2 = prog.render(1)
        img, st3 = prog.render(77)
    assert same_bits(img, ref)
    assert tuple(a + b + c for a, b, c in zip(counts(st1), counts(st2), counts(st3))) == counts(rst)


# ---- 5. borders and lists ---------------------------------------------------------------------

@pytest.mark.parametrize("w,h", [(20, 11), (7, 3)])
def test_clipped_tiles(scene_dir, w, h):
    s = load(scene_dir, "bunny.sp", w, h, bvh=1)
    ref, rst = one_shot(s, "direct_lighting", 6)
    with sp.Progressive(s, "direct_lighting") as prog:
        img, total = run_passes(prog, (2, 1, 3))
        state, n = prog.export_state()
    assert same_bits(img, ref) and total == counts(rst)
    raw = state.view(np.uint8).reshape(-1, sp.PIXEL_STATE_DTYPE.itemsize)
    outside = 0
    for slot in range(img.shape[0]):
        for m in range(64):
            x, y = pixel_xy(w, slot, m)
            if x >= w or y >= h:
                outside += 1
                assert not img[slot, m].any() and not raw[slot * 64 + m].any(), (slot, m)
            else:
                assert raw[slot * 64 + m].any(), (slot, m)
    assert outside == img.shape[0] * 64 - w * h and outside > 0


def test_shuffled_list_with_duplicates(scene_dir):
    # every slot carries its own state: a tile listed twice advances twice, each from its own record
    s = load(scene_dir, "bunny.sp", 72, 40, bvh=1)
    n = sp.TileScheduler(72, 40).get_num_tiles()
    ref, _ = one_shot(s, "direct_lighting", 7)
    ids = np.random.default_rng(5).permutation(n)[:17].astype(np.int32)
    ids = np.concatenate([ids, ids[:4], ids[2:3]])
    with sp.Progressive(s, "direct_lighting", ids) as prog:
        img, _ = run_passes(prog, (3, 4))
    assert same_bits(img, ref[ids])


def test_device_tile_list(scene_dir):
    s = load(scene_dir, "bunny.sp", 72, 40, bvh=1)
    n = sp.TileScheduler(72, 40).get_num_tiles()
    good = np.array([3, 0, n - 1], dtype=np.int32)
    ref, rst = one_shot(s, "direct_lighting", 5, good)
    ids = np.array([3, -1, 0, n, n - 1], dtype=np.int32)  # a device list is not checked: outside ids render zeros
    d = torch.from_numpy(ids).cuda()
    with sp.Progressive(s, "direct_lighting", d_tile_ids=d.data_ptr(), num_tiles=ids.size) as prog:
        d.fill_(0)  # the list was copied at creation
        torch.cuda.synchronize()
        img, total = run_passes(prog, (2, 3))
        state, _ = prog.export_state()
    assert same_bits(img[[0, 2, 4]], ref) and not img[[1, 3]].any()
    assert total == counts(rst)
    raw = state.view(np.uint8).reshape(ids.size, 64, -1)
    assert not raw[[1, 3]].any() and raw[[0, 2, 4]].any(axis=2).all()


# ---- 6. the state is the reference sampler's --------------------------------------------------

def test_exported_state_is_std_mt19937_64(scene_dir, tmp_path):
    exe = str(tmp_path / "mt_continue_check")
    subprocess.run(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "cpp", "mt_continue_check.cpp"), "-o", exe],
                   check=True, timeout=300)
    w, h = 64, 40
    s = load(scene_dir, "bunny.sp", w, h, bvh=1)
    rec = np.dtype([("seed", "<u8"), ("draws", "<u8"), ("mt", "<u8", (312,)), ("mt_pos", "<u8")])
    assert rec.itemsize == 8 * 315

    def check(prog, tag):
        state, n = prog.export_state()
        out = np.zeros(w * h, dtype=rec)
        k = 0
        for slot in range(prog.num_tiles):
            for m in range(64):
                x, y = pixel_xy(w, slot, m)
                if x < w and y < h:
                    r = state[slot * 64 + m]
                    out[k] = (((x << 16) | y) ^ 0xb0ae9d99, r["draws"], r["mt"], r["mt_pos"])
                    k += 1
        assert k == w * h
        path = str(tmp_path / f"state_{tag}.bin")
        out.tofile(path)
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and f"{w * h} records, 0 mismatching" in r.stdout, r.stdout + r.stderr
        edge = int(np.sum((out["mt_pos"] == 0) | (out["mt_pos"] == 312)))
        print(f"{tag}: {n} samples, {edge} of {w * h} pixels at a generation boundary (mt_pos 0 or 312), "
              f"{int(np.sum(out['draws'] == 0))} with no draws")
        return edge

    with sp.Progressive(s, "direct_lighting") as prog:
        # before any sample: the seeded engine, position 312
        state0, n0 = prog.export_state()
        assert n0 == 0 and int(state0["mt_pos"].max()) == 312 and int(state0["draws"].max()) == 0
        check(prog, "seeded")
        prog.render(3)
        prog.render(4)
        edge = check(prog, "3+4")
        if edge == 0:  # (one more pass of one sample, as the only retry)
            prog.render(1)
            edge = check(prog, "3+4+1")
        assert edge > 0


# ---- 7. checkpoint round trip -----------------------------------------------------------------

def test_checkpoint_round_trip(scene_dir):
    path = os.path.join(scene_dir, "bunny.sp")
    s = load(scene_dir, "bunny.sp", 64, 40, bvh=1)
    ref, rst = one_shot(s, "direct_lighting", 8)
    prog = sp.Progressive(s, "direct_lighting")
    _, st3 = prog.render(3)
    state, n = prog.export_state()
    prog.close()
    assert n == 3
    del s
    # a new scene handle of the same file
    s2 = sp.Scene.from_file(path)
    s2.set_resolution(64, 40)
    s2.upload(device=0, bvh_mode=1)
    prog = sp.Progressive(s2, "direct_lighting")
    L = sp.lib()
    # refused imports leave the object as it was
    bad_pos = state.copy()
    bad_pos["mt_pos"][5] = 313
    bad_res = state.copy()
    bad_res["reserved"][9] = 1
    for arr, count in ((state[:-1], state.size - 1), (bad_pos, state.size), (bad_res, state.size)):
        a = np.ascontiguousarray(arr)
        assert L.sp_progress_import(prog._h, C.c_void_p(a.ctypes.data), count, 3) == _abi.SP_ERR_ARG
    small = np.zeros(state.size - 64, dtype=sp.PIXEL_STATE_DTYPE)
    got = C.c_uint32()
    assert L.sp_progress_export(prog._h, C.c_void_p(small.ctypes.data), small.size, C.byref(got)) == _abi.SP_ERR_ARG
    assert prog.samples == 0
    prog.import_state(state, n)
    assert prog.samples == 3
    img, st5 = prog.render(5)
    assert same_bits(img, ref)
    assert tuple(a + b for a, b in zip(counts(st3), counts(st5))) == counts(rst)
    # the draws carried through the checkpoint
    state8, n8 = prog.export_state()
    assert n8 == 8 and int(state8["draws"].sum()) == rst.rng_draws
    # ... and the object still renders correctly after the refused calls
    with pytest.raises(sp.SimplePathError):
        prog.render(0)
    img9, _ = prog.render(1)
    assert same_bits(img9, one_shot(s2, "direct_lighting", 9)[0])
    prog.close()


# ---- 8. stream order and lifetime -------------------------------------------------------------

def test_stream_ordered_passes_and_dependent_kernel(scene_dir):
    s = load(scene_dir, "bunny.sp", 256, 160)
    ref8, _ = one_shot(s, "direct_lighting", 8)
    ref16, _ = one_shot(s, "direct_lighting", 16)
    dev = torch.device("cuda:0")
    out_a = torch.zeros((ref8.shape[0], 64, 3), dtype=torch.float32, device=dev)
    out_b = torch.zeros_like(out_a)
    prog = sp.Progressive(s, "direct_lighting")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for out in (out_a, out_b):
            assert prog.render(8, out.data_ptr(), stream.cuda_stream, stats=False) == (None, None)
        busy = not stream.query()  # only enqueued: the stream still has work
        both = out_a + out_b       # a dependent kernel behind them, still without a host wait
    stream.synchronize()
    assert busy, "sp_progress_render waited for the render although no stats were requested"
    assert prog.samples == 16
    assert same_bits(out_a.cpu().numpy(), ref8) and same_bits(out_b.cpu().numpy(), ref16)
    assert np.array_equal(both.cpu().numpy(), ref8 + ref16)
    # accumulate only (no image), then the image of everything
    prog.render(3, 0, None)
    img, _ = prog.render(1)
    assert same_bits(img, one_shot(s, "direct_lighting", 20)[0])
    prog.close()


def test_scene_changes_invalidate_the_object(scene_dir):
    s = load(scene_dir, "bunny.sp", 64, 40)
    prog = sp.Progressive(s, "direct_lighting")
    n = prog.num_tiles
    assert abs(prog.device_bytes - n * 64 * 2528) <= 0.01 * n * 64 * 2528
    prog.render(2)
    s.upload(device=0, bvh_mode=0)  # the same options: nothing is uploaded again
    prog.render(1)
    s.set_resolution(64, 40)
    for call in (lambda: prog.render(1), prog.export_state):
        with pytest.raises(sp.SimplePathError) as e:
            call()
        assert e.value.code == _abi.SP_ERR_STATE
    prog.close()
    prog = sp.Progressive(s, "direct_lighting")
    s.upload(device=0, bvh_mode=1)  # other options: the device scene is rebuilt
    with pytest.raises(sp.SimplePathError) as e:
        prog.render(1)
    assert e.value.code == _abi.SP_ERR_STATE
    prog.close()
    with pytest.raises(sp.SimplePathError) as e:
        sp.Progressive(s, "whitted", waves_per_simd=3)
    assert e.value.code == _abi.SP_ERR_ARG


def test_forced_tile_order_is_invisible(scene_dir):
    # more tiles than persistent waves, the probe's order kept from the first call on
    s = load(scene_dir, "bunny.sp", 640, 512)
    ref, rst = one_shot(s, "direct_lighting", 3, tile_order_factor=-1.0)
    with sp.Progressive(s, "direct_lighting", tile_order_factor=2.0) as prog:
        _, st1 = prog.render(1)
        img, st2 = prog.render(2)
        assert abs(prog.device_bytes - prog.num_tiles * 64 * 2528) <= 0.01 * prog.num_tiles * 64 * 2528
    assert (st1.launches, st2.launches) == (3, 1)
    assert same_bits(img, ref)
    assert tuple(a + b for a, b in zip(counts(st1), counts(st2))) == counts(rst)


# ---- 9. existing paths untouched --------------------------------------------------------------

def test_one_shot_renders_unchanged_beside_a_progress_object(scene_dir):
    s = load(scene_dir, "bunny.sp", 64, 40)
    before, bst = sp.render_tiles(s, "direct_lighting", 8)
    with sp.Progressive(s, "direct_lighting") as prog:
        prog.render(3)
        mid, mst = sp.render_tiles(s, "direct_lighting", 8)
        img, _ = prog.render(5)
    after, ast = sp.render_tiles(s, "direct_lighting", 8)
    assert same_bits(before, mid) and same_bits(before, after) and same_bits(img, before)
    assert counts(bst) == counts(mst) == counts(ast)
    assert (bst.pipeline, bst.launches) == (ast.pipeline, ast.launches)
