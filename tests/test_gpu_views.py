"""Many views in one launch (sp_render_views, include/simplepath_hip.h): view v is, bit for bit, the
image sp_render_tiles gives for the same tiles, integrator and samples after set_camera(cameras[v]),
and the counts are the sums of those calls'.

The corners: one view against the one-shot kernel for every integrator (closed_room's depth 40 runs
the deep-recursion buffer); clipped border tiles and a tile list with its own slots; an image light,
whose draw counts depend on the data; waves that leave one view's items for the next view's, where a
camera kept across items would show; host against device cameras; stream order; the scene's own
camera and its progress objects, which a views call leaves alone; and the C++ header's wrappers."""
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
CAMERA_INTEGRATORS = ["brute_force", "brute_force_iterative", "brute_force_iterative_rr", "iterative_rrnee",
                      "direct_lighting", "whitted"]


def load(scene_dir, name, w, h, bvh=0, upload=True):
    s = sp.Scene.from_file(os.path.join(scene_dir, name))
    s.set_resolution(w, h)
    if upload:
        s.upload(device=0, bvh_mode=bvh)
    return s


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def counts(st):
    return (st.rays, st.shadow_rays, st.samples, st.rng_draws)


def one_shot(s, integrator, spp, ids=None, **kw):
    return sp.render_tiles(s, integrator, spp, ids, pipeline="megakernel", tail_fraction=-1.0, **kw)


def edited(cam, shift=(0.0, 0.0), zoom=1.0):
    """a camera sheared by `shift` pixels and zoomed out by `zoom`: valid for any scene's scale"""
    c = _abi.sp_camera_desc.from_buffer_copy(cam)
    t = c.transform
    f = np.float32
    for k in range(3):
        t.vz[k] = f(t.vz[k]) + f(shift[0]) * f(t.vx[k]) + f(shift[1]) * f(t.vy[k])
        t.vx[k] = f(zoom) * f(t.vx[k])
        t.vy[k] = f(zoom) * f(t.vy[k])
    return c


def three_cameras(s):
    own = _abi.sp_camera_desc.from_buffer_copy(s.desc().camera)
    return [own, edited(own, (3.0, -2.0), 1.25), edited(own, (-1.5, 0.75), 0.75)]


def floats12(cams):
    return np.array([[*c.transform.vx, *c.transform.vy, *c.transform.vz, *c.transform.p] for c in cams], dtype=np.float32)


def single_views(s, integrator, spp, cams, ids=None, **kw):
    """the comparison: set_camera + render_tiles per camera, the scene's own camera put back"""
    own = _abi.sp_camera_desc.from_buffer_copy(s.desc().camera)
    imgs, total = [], np.zeros(4, dtype=np.int64)
    for c in cams:
        s.set_camera(c)
        img, st = one_shot(s, integrator, spp, ids, **kw)
        imgs.append(img)
        total += np.array(counts(st), dtype=np.int64)
    s.set_camera(own)
    return imgs, tuple(int(x) for x in total)


# ---- one view is the one-shot render ------------------------------------------------------------

@pytest.mark.parametrize("integrator", CAMERA_INTEGRATORS)
def test_one_view_equals_render_tiles(scene_dir, integrator):
    s = load(scene_dir, "closed_room.sp", 40, 24)
    ref, rst = one_shot(s, integrator, 8)
    img, st = sp.render_views(s, integrator, 8, [s.desc().camera])
    assert img.shape == (1, 15, 64, 3)
    assert same_bits(img[0], ref)
    assert counts(st) == counts(rst)
    assert (st.pipeline, st.launches) == (sp.PIPELINES["megakernel"], 1)


# ---- three cameras, clipped tiles, a list with its own slots -------------------------------------

@pytest.mark.parametrize("per_lane", [False, True])
@pytest.mark.parametrize("integrator", ["direct_lighting", "iterative_rrnee"])
@pytest.mark.parametrize("scene_name,bvh", [("elf_small.sp", 0), ("bunny.sp", 1)])
def test_three_cameras_match_the_oracle(scene_dir, scene_name, bvh, integrator, per_lane):
    s = load(scene_dir, scene_name, 20, 12, bvh=bvh)  # 3 x 2 tiles, clipped on the right and at the bottom
    host = load(scene_dir, scene_name, 20, 12, upload=False)  # the oracle's scene
    ids = [5, 0, 3]
    cams = three_cameras(s)
    img, st = sp.render_views(s, integrator, 5, cams, ids, per_lane_queries=per_lane)
    assert img.shape == (3, 3, 64, 3)
    total = np.zeros(3, dtype=np.int64)
    for v, c in enumerate(cams):
        host.set_camera(c)
        ref, rst = _oracle.render(host, sp.string_to_integrator_type(integrator), 5, ids, variant="spm")
        print(scene_name, integrator, "view", v, "differing values", int(np.sum(img[v].view(np.uint32) != ref.view(np.uint32))))
        assert same_bits(img[v], ref), v
        total += np.array([rst["rays"], rst["shadow_rays"], rst["samples"]], dtype=np.int64)
    assert not same_bits(img[0], img[1]) and not same_bits(img[1], img[2])
    assert (st.rays, st.shadow_rays, st.samples) == tuple(int(x) for x in total)
    # ... and the device's own single-view calls, whose draw counts the oracle does not report
    imgs, gpu_total = single_views(s, integrator, 5, cams, ids, per_lane_queries=per_lane)
    assert all(same_bits(img[v], imgs[v]) for v in range(3))
    assert counts(st) == gpu_total


def test_image_light_draw_counts(scene_dir):
    s = load(scene_dir, "material_spheres_ibl.sp", 24, 16)
    host = load(scene_dir, "material_spheres_ibl.sp", 24, 16, upload=False)
    cams = three_cameras(s)
    img, st = sp.render_views(s, "direct_lighting", 5, cams)
    imgs, total = single_views(s, "direct_lighting", 5, cams)
    for v, c in enumerate(cams):
        host.set_camera(c)
        ref, _ = _oracle.render(host, sp.string_to_integrator_type("direct_lighting"), 5, variant="spm")
        assert same_bits(img[v], ref) and same_bits(img[v], imgs[v]), v
    assert counts(st) == total


# ---- waves that cross from one view into the next --------------------------------------------------

@pytest.mark.parametrize("waves,spp", [(0, 1), (1, 2)])
def test_waves_cross_from_view_to_view(scene_dir, waves, spp):
    s = load(scene_dir, "lucy_small.sp", 16, 16)  # 4 tiles per view
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    # at most 16 waves per CU are resident: with twice as many items every wave takes several, and
    # with 4 items per view consecutive items of a wave belong to different views
    n_views = -(-(2 * 16 * cus) // 4)
    n_views += (-n_views) % 3
    assert n_views % 3 == 0 and 4 * n_views >= 2 * 16 * cus and 4 * (n_views - 3) < 2 * 16 * cus
    cams = three_cameras(s)
    refs, ref_total = single_views(s, "direct_lighting", spp, cams, waves_per_simd=waves)
    d_cams = torch.from_numpy(floats12([cams[v % 3] for v in range(n_views)])).cuda()
    out = torch.full((n_views, 4, 64, 3), float("nan"), dtype=torch.float32, device="cuda")
    st = sp.render_views_device(s, "direct_lighting", spp, None, None, out.data_ptr(), d_cameras=d_cams.data_ptr(),
                                num_views=n_views, waves_per_simd=waves)
    img = out.cpu().numpy()
    for k in range(3):
        want = np.broadcast_to(refs[k], img[k::3].shape)
        wrong = np.flatnonzero(np.any(img[k::3].view(np.uint32) != want.view(np.uint32), axis=(1, 2, 3)))
        assert wrong.size == 0, (k, wrong[:8] * 3 + k)
    assert not same_bits(refs[0], refs[1]) and not same_bits(refs[1], refs[2])
    assert counts(st) == tuple(x * (n_views // 3) for x in ref_total)
    assert st.launches == 1


# ---- host and device cameras, stream order ------------------------------------------------------------

def test_host_and_device_cameras_give_equal_bytes(scene_dir):
    s = load(scene_dir, "bunny.sp", 20, 12)
    cams = three_cameras(s)
    ids = [5, 0, 3]
    host_img, host_st = sp.render_views(s, "direct_lighting", 3, cams, ids)
    d_cams = torch.from_numpy(floats12(cams)).cuda()
    d_ids = torch.tensor(ids, dtype=torch.int32, device="cuda")
    out = torch.zeros((3, 3, 64, 3), dtype=torch.float32, device="cuda")
    st = sp.render_views_device(s, "direct_lighting", 3, None, None, out.data_ptr(), d_cameras=d_cams.data_ptr(), num_views=3,
                                d_tile_ids=d_ids.data_ptr(), num_tiles=3)
    assert same_bits(out.cpu().numpy(), host_img) and counts(st) == counts(host_st)
    out.zero_()
    st = sp.render_views_device(s, "direct_lighting", 3, cams, ids, out.data_ptr())  # host cameras, device image
    assert same_bits(out.cpu().numpy(), host_img) and counts(st) == counts(host_st)


def test_stream_order(scene_dir):
    s = load(scene_dir, "bunny.sp", 20, 12)
    cams = three_cameras(s)
    ref_a, _ = sp.render_views(s, "direct_lighting", 3, cams)
    ref_b, _ = sp.render_views(s, "direct_lighting", 2, cams[::-1], [4, 1])
    a = torch.zeros((3, 6, 64, 3), dtype=torch.float32, device="cuda")
    b = torch.zeros((3, 2, 64, 3), dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        h = stream.cuda_stream
        assert sp.render_views_device(s, "direct_lighting", 3, cams, None, a.data_ptr(), stream=h, stats=False) is None
        # the second call's host cameras and tile list are staged while the first is queued
        assert sp.render_views_device(s, "direct_lighting", 2, cams[::-1], [4, 1], b.data_ptr(), stream=h, stats=False) is None
    stream.synchronize()
    assert same_bits(a.cpu().numpy(), ref_a) and same_bits(b.cpu().numpy(), ref_b)


# ---- what a views call leaves alone ------------------------------------------------------------------

def test_scene_camera_and_progress_objects_are_left_alone(scene_dir):
    s = load(scene_dir, "bunny.sp", 20, 12)
    cams = three_cameras(s)
    own = bytes(s.desc().camera)
    before, bst = one_shot(s, "direct_lighting", 4)
    with sp.Progressive(s, "direct_lighting") as prog:
        prog.render(1)
        img, _ = sp.render_views(s, "direct_lighting", 2, cams[1:])
        assert not same_bits(img[0], img[1])
        final, _ = prog.render(3)  # still valid: the generation did not move
    assert same_bits(final, before)
    assert bytes(s.desc().camera) == own
    after, ast = one_shot(s, "direct_lighting", 4)
    assert same_bits(after, before) and counts(ast) == counts(bst)


def test_refusals_on_a_resident_scene(scene_dir):
    s = load(scene_dir, "bunny.sp", 20, 12)
    cam = s.desc().camera
    with pytest.raises(sp.SimplePathError) as e:
        sp.render_views(s, "mandelbrot", 2, [cam])
    assert e.value.code == _abi.SP_ERR_UNSUPPORTED
    # more queue items than the int32 queue head counts: refused before anything is touched
    with pytest.raises(sp.SimplePathError) as e:
        sp.render_views_device(s, "direct_lighting", 1, None, None, 0x1000, d_cameras=0x1000, num_views=2 ** 31 - 1,
                               d_tile_ids=0x1000, num_tiles=2)
    assert e.value.code == _abi.SP_ERR_UNSUPPORTED
    with pytest.raises(sp.SimplePathError) as e:
        sp.render_views(s, "whitted", 2, [cam], waves_per_simd=3)  # as sp_render_tiles
    assert e.value.code == _abi.SP_ERR_ARG


# ---- the C++ header ------------------------------------------------------------------------------

def read_pfm(path):
    with open(path, "rb") as fh:
        assert fh.readline().strip() == b"PF"
        w, h = (int(x) for x in fh.readline().split())
        scale = float(fh.readline())
        data = np.frombuffer(fh.read(), dtype="<f4" if scale < 0 else ">f4")
    return data.reshape(h, w, 3)[::-1]  # rows bottom-up in the file (Image/Image.cpp:40)


def test_cpp_program_matches_python(scene_dir, tmp_path):
    exe = os.path.join(ROOT, "tests", "cpp", "_build", "views_main")
    assert os.path.exists(exe), "tests/cpp/views.mk builds it (__graft_entry__.build)"
    path = os.path.join(scene_dir, "bunny.sp")
    views = [((0.0, 2.0, 5.0), (-0.25, 1.0, 0.0), 45.0), ((2.5, 1.75, 3.5), (-0.25, 0.75, 0.0), 38.0)]
    prefix = str(tmp_path / "view")
    args = [exe, path, "--size", "48", "32", "--spp", "3", "--output", prefix]
    for eye, look, fov in views:
        args += ["--view", *(repr(x) for x in (*eye, *look, fov))]
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    s = load(scene_dir, "bunny.sp", 48, 32)
    cams = [sp.camera_look_at(eye, look, (0.0, 1.0, 0.0), fov, 48, 32) for eye, look, fov in views]
    assert bytes(cams[0]) == bytes(s.desc().camera)  # the first is the scene file's own
    img, st = sp.render_views(s, "direct_lighting", 3, cams)
    assert f"views 2 rays {st.rays} launches 1" in r.stdout
    for v in range(2):
        assert same_bits(read_pfm(prefix + f"{v}.pfm"), sp.tiles_to_image(48, 32, img[v])), v
    assert same_bits(read_pfm(prefix + "_set.pfm"), sp.tiles_to_image(48, 32, img[1]))
