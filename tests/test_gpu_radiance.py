"""Radiance queries (sp_scene_radiance_rays, include/simplepath_hip.h): record i is the reference's
Integrator::integrate along the caller's ray with a sampler seeded by the record, called N times,
summed and divided.  Every comparison is bitwise and no record is left out.

The oracle needs no change: a camera with vx = vy = 0, vz = D, p = O makes every pixel sample's ray
(O, normalize(D)), since (fx * 0 + fy * 0) + D = D.  Under that camera the CPU oracle's pixel (x, y)
is integrate along that one ray with the sampler seeded pixel_seed(x, y), N calls summed and divided
-- a record's meaning exactly.  render_tiles under the same camera (megakernel, no tail chunks) is the
second reference: the same walk, so equal-distance ties agree, and it reports rng_draws.

The corners: every integrator that has a ray (closed_room's depth 40 runs the deep-recursion buffer),
both BVH modes; different rays in one wave; an image light, whose draw counts depend on the data; a
queue long enough that every wave takes several items and the last one is partial; rays no integrator
makes; what a query leaves alone and what it sees; refusals on a resident scene."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import simplepath_amd as sp
from simplepath_amd import _abi
from tests import _lbvh_sets, _oracle, _refit_moves as R

pytestmark = pytest.mark.gpu

F = np.float32
RAY_INTEGRATORS = ["brute_force", "brute_force_iterative", "brute_force_iterative_rr", "iterative_rrnee",
                   "direct_lighting", "whitted"]
N = 5
# closed_room.sp: the camera's place; into the clearcoat-on-glossy ball, into a lambertian wall, into
# the sphere light (nothing leaves a closed room).  No component is zero.
ROOM_O = (0.0, 0.0, 0.0)
ROOM_D = [(0.1, -0.9, -3.6), (1.0, 0.3, -0.5), (0.05, 1.45, -3.0)]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def counts(st):
    return (st.rays, st.shadow_rays, st.samples, st.rng_draws)


def one_shot(s, integrator, spp, **kw):
    return sp.render_tiles(s, integrator, spp, None, pipeline="megakernel", tail_fraction=-1.0, **kw)


def unit(D):
    """normalize(D) as the oracle's camera computes it, in float32: D * rsqrt((x x + y y) + (z z + 0))"""
    x, y, z = (F(v) for v in D)
    assert x != 0 and y != 0 and z != 0
    dot = F(F(x * x) + F(y * y)) + F(F(z * z) + F(0.0))
    r = F(_oracle.load("spm").orc_rsqrt(float(dot)))
    return np.array([x * r, y * r, z * r], dtype=F)


def staring(scene, O, D):
    """the scene's camera with vx = vy = 0, vz = D, p = O: every pixel looks along D from O"""
    c = _abi.sp_camera_desc.from_buffer_copy(scene.desc().camera)
    for k in range(3):
        c.transform.vx[k] = c.transform.vy[k] = 0.0
        c.transform.vz[k] = float(F(D[k]))
        c.transform.p[k] = float(F(O[k]))
    return c


def tile_pixels(w, h):
    """(x, y) of tile-packed record slot * 64 + m for a whole w x h frame of full tiles"""
    assert w % 8 == 0 and h % 8 == 0
    m = np.arange(64)
    dx = (m & 1) | (((m >> 2) & 1) << 1) | (((m >> 4) & 1) << 2)
    dy = ((m >> 1) & 1) | (((m >> 3) & 1) << 1) | (((m >> 5) & 1) << 2)
    t = np.arange((w // 8) * (h // 8))
    x = ((t % (w // 8)) * 8)[:, None] + dx[None, :]
    y = ((t // (w // 8)) * 8)[:, None] + dy[None, :]
    return x.ravel(), y.ravel()


def records(O, D, w, h):
    """one record per pixel of the frame in tile-packed order: the ray (O, unit(D)), the pixel's seed"""
    x, y = tile_pixels(w, h)
    n = x.size
    return sp.make_radiance_rays(np.tile(np.asarray(O, dtype=F), (n, 1)), np.tile(unit(D), (n, 1)), sp.pixel_seed(x, y))


def fields(rays):
    return rays["o"], rays["d"], rays["seed"]


_SCENES, _REFS = {}, {}


def room(scene_dir, bvh):
    """(resident closed_room at 16 x 8, its host twin for the oracle), one pair per bvh_mode"""
    if bvh not in _SCENES:
        pair = []
        for upload in (True, False):
            s = sp.Scene.from_file(os.path.join(scene_dir, "closed_room.sp"))
            s.set_resolution(16, 8)  # 2 tiles, 128 seeds
            if upload:
                s.upload(device=0, bvh_mode=bvh)
            pair.append(s)
        _SCENES[bvh] = tuple(pair)
    return _SCENES[bvh]


def room_refs(scene_dir, integrator, bvh, spp=N):
    """per ray of ROOM_D: (oracle image [128, 3], oracle counts, render_tiles counts); computed once"""
    key = (integrator, bvh, spp)
    if key not in _REFS:
        s, host = room(scene_dir, bvh)
        out = []
        for D in ROOM_D:
            cam = staring(s, ROOM_O, D)
            host.set_camera(cam)
            img, ost = _oracle.render(host, sp.string_to_integrator_type(integrator), spp, variant="spm")
            s.set_camera(cam)
            gpu, gst = one_shot(s, integrator, spp)
            assert same_bits(gpu, img), "the second reference disagrees with the first"
            img = img.reshape(-1, 3).copy()
            img.setflags(write=False)
            out.append((img, (ost["rays"], ost["shadow_rays"], ost["samples"]), counts(gst)))
        _REFS[key] = out
    return _REFS[key]


def room_records(k):
    return records(ROOM_O, ROOM_D[k], 16, 8)


# ---- 1. every integrator that has a ray --------------------------------------------------------------

@pytest.mark.parametrize("integrator,bvh", [(i, 0) for i in RAY_INTEGRATORS] + [("direct_lighting", 1), ("iterative_rrnee", 1)])
def test_every_integrator_matches_the_oracle(scene_dir, integrator, bvh):
    s, _ = room(scene_dir, bvh)
    refs = room_refs(scene_dir, integrator, bvh)
    for k, (img, ocnt, gcnt) in enumerate(refs):
        out, st = s.radiance(*fields(room_records(k)), integrator, N)
        print(integrator, bvh, "ray", k, "differing values", int(np.sum(out.view(np.uint32) != img.view(np.uint32))), counts(st))
        assert out.shape == (128, 3) and same_bits(out, img), k
        assert counts(st)[:3] == ocnt, k
        assert counts(st) == gcnt, k
        assert (st.pipeline, st.launches) == (sp.PIPELINES["megakernel"], 1)
    # the three rays see different things, and none of them nothing
    assert not same_bits(refs[0][0], refs[1][0]) and not same_bits(refs[1][0], refs[2][0])
    assert all(r[0].max() > 0.0 for r in refs)


# ---- 2. different rays in one wave -------------------------------------------------------------------

@pytest.mark.parametrize("per_lane", [False, True])
@pytest.mark.parametrize("integrator", ["direct_lighting", "iterative_rrnee"])
def test_shuffled_rays_give_shuffled_results(scene_dir, integrator, per_lane):
    s, _ = room(scene_dir, 0)
    refs = room_refs(scene_dir, integrator, 0)
    rays = np.concatenate([room_records(k) for k in range(3)])
    want = np.concatenate([r[0] for r in refs])
    perm = np.random.default_rng(20).permutation(rays.shape[0])
    out, st = s.radiance(*fields(rays[perm]), integrator, N, per_lane_queries=per_lane)
    wrong = np.flatnonzero(np.any(out.view(np.uint32) != want[perm].view(np.uint32), axis=1))
    assert wrong.size == 0, (wrong[:8], perm[wrong[:8]])
    assert counts(st) == tuple(sum(r[2][c] for r in refs) for c in range(4))


# ---- 3. an image light: draw counts that depend on the data --------------------------------------------

def test_image_light_draw_counts(scene_dir):
    path = os.path.join(scene_dir, "material_spheres_ibl.sp")
    s, host = sp.Scene.from_file(path), sp.Scene.from_file(path)
    for x in (s, host):
        x.set_resolution(8, 8)
    s.upload(device=0)
    t = s.desc().camera.transform
    vx, vy, vz, p = (np.array(list(a), dtype=F) for a in (t.vx, t.vy, t.vz, t.p))
    draws = 0
    rays, want = [], []
    for fx, fy in ((3.25, 4.5), (0.75, 0.5)):  # near the frame's middle, and its top left corner
        D = (F(fx) * vx + F(fy) * vy + vz).astype(F)
        cam = staring(s, p, D)
        host.set_camera(cam)
        img, ost = _oracle.render(host, sp.string_to_integrator_type("direct_lighting"), N, variant="spm")
        s.set_camera(cam)
        gpu, gst = one_shot(s, "direct_lighting", N)
        rec = records(p, D, 8, 8)
        out, st = s.radiance(*fields(rec), "direct_lighting", N)
        assert same_bits(out, img.reshape(-1, 3)) and same_bits(gpu, img)
        assert counts(st)[:3] == (ost["rays"], ost["shadow_rays"], ost["samples"]) and counts(st) == counts(gst)
        draws += gst.rng_draws
        rays.append(rec)
        want.append(img.reshape(-1, 3))
    assert not same_bits(want[0], want[1])
    out, st = s.radiance(*fields(np.concatenate(rays)), "direct_lighting", N)
    assert same_bits(out, np.concatenate(want)) and st.rng_draws == draws


# ---- 4. the queue ------------------------------------------------------------------------------------

@pytest.mark.parametrize("integrator,waves", [("direct_lighting", 0), ("direct_lighting", 1), ("iterative_rrnee", 2)])
def test_every_wave_takes_several_items(scene_dir, integrator, waves):
    s, _ = room(scene_dir, 0)
    base = np.concatenate([room_records(k) for k in range(3)])  # 384 records
    first, fst = s.radiance(*fields(base), integrator, 2, waves_per_simd=waves)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 64 * (8 * cus) + 37  # at most 16 waves per CU are resident, often 8: each takes several items
    rays = np.resize(base, n)
    d_rays = torch.from_numpy(rays.view(np.int32).reshape(n, 8)).cuda()
    guard = 0x7fc12345
    out = torch.full((n * 3 + 64,), guard, dtype=torch.int32, device="cuda")
    st = s.radiance_device(d_rays.data_ptr(), n, out.data_ptr(), integrator, 2, waves_per_simd=waves)
    got = out.cpu().numpy().view(np.uint32)
    assert np.all(got[n * 3:] == guard)
    got = got[:n * 3].reshape(n, 3)
    want = first.view(np.uint32)[np.arange(n) % base.shape[0]]
    wrong = np.flatnonzero(np.any(got != want, axis=1))
    assert wrong.size == 0, wrong[:8]
    q, r = divmod(n, base.shape[0])
    assert st.samples == 2 * n and st.launches == 1
    part, pst = (s.radiance(*fields(base[:r]), integrator, 2, waves_per_simd=waves) if r else (None, None))
    tail = counts(pst) if r else (0, 0, 0, 0)
    assert counts(st) == tuple(q * a + b for a, b in zip(counts(fst), tail))


# ---- 5. rays no integrator makes -----------------------------------------------------------------------

@pytest.mark.parametrize("integrator", ["direct_lighting", "iterative_rrnee", "brute_force"])
def test_rays_no_integrator_makes(scene_dir, integrator):
    s, _ = room(scene_dir, 0)
    img = room_refs(scene_dir, integrator, 0)[0][0]
    rays = room_records(0).copy()
    bad = [3, 64, 100, 127]
    rays["o"][3, 0] = np.nan
    rays["d"][64, 1] = np.inf
    rays["d"][100] = (0.0, -0.0, 0.0)
    rays["o"][127, 2] = -np.inf
    out, st = s.radiance(*fields(rays), integrator, N)
    assert np.all(out.view(np.uint32)[bad] == 0)  # +0.0
    ok = np.setdiff1d(np.arange(128), bad)
    assert same_bits(out[ok], img[ok])
    alone, ast = s.radiance(*fields(rays[ok]), integrator, N)
    assert same_bits(alone, img[ok])
    assert counts(st) == counts(ast) and st.samples == N * ok.size
    # nothing but such rays: a launch that walks nothing
    out, st = s.radiance(*fields(rays[bad]), integrator, N)
    assert np.all(out.view(np.uint32) == 0) and counts(st) == (0, 0, 0, 0)


# ---- 6. scene state and order --------------------------------------------------------------------------

def as_device(rays):
    return torch.from_numpy(rays.view(np.int32).reshape(-1, 8).copy()).cuda()


def test_stream_order_and_host_equals_device(scene_dir):
    s, _ = room(scene_dir, 0)
    s.set_camera(staring(s, ROOM_O, ROOM_D[1]))
    ra, rb = room_records(0), room_records(2)
    ref_a, ast = s.radiance(*fields(ra), "direct_lighting", N)
    ref_b, _ = s.radiance(*fields(rb), "iterative_rrnee", 3)
    ref_c, _ = one_shot(s, "direct_lighting", 3)
    da, db = as_device(ra), as_device(rb)
    a = torch.zeros((128, 3), dtype=torch.float32, device="cuda")
    b = torch.zeros((128, 3), dtype=torch.float32, device="cuda")
    c = torch.zeros((2, 64, 3), dtype=torch.float32, device="cuda")
    # host form equals device form, counts included
    st = s.radiance_device(da.data_ptr(), 128, a.data_ptr(), "direct_lighting", N)
    assert same_bits(a.cpu().numpy(), ref_a) and counts(st) == counts(ast)
    a.zero_()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        h = stream.cuda_stream
        assert s.radiance_device(da.data_ptr(), 128, a.data_ptr(), "direct_lighting", N, stream=h, stats=False) is None
        assert sp.render_tiles_device(s, "direct_lighting", 3, None, c.data_ptr(), stream=h, pipeline="megakernel",
                                      tail_fraction=-1.0, stats=False) is None
        assert s.radiance_device(db.data_ptr(), 128, b.data_ptr(), "iterative_rrnee", 3, stream=h, stats=False) is None
    stream.synchronize()
    assert same_bits(a.cpu().numpy(), ref_a) and same_bits(b.cpu().numpy(), ref_b) and same_bits(c.cpu().numpy(), ref_c)


def test_camera_and_progress_objects_are_left_alone(scene_dir):
    s, _ = room(scene_dir, 0)
    s.set_camera(staring(s, ROOM_O, ROOM_D[0]))
    rays = room_records(1)
    before, bst = one_shot(s, "direct_lighting", 4)
    own = bytes(s.desc().camera)
    with sp.Progressive(s, "direct_lighting") as prog:
        prog.render(1)
        one, ost = s.radiance(*fields(rays), "direct_lighting", N)
        final, _ = prog.render(3)  # still valid
    assert same_bits(final, before) and bytes(s.desc().camera) == own
    s.set_camera(staring(s, (0.5, 0.25, -1.0), ROOM_D[2]))  # a query does not read the camera
    two, tst = s.radiance(*fields(rays), "direct_lighting", N)
    assert same_bits(one, two) and counts(ost) == counts(tst)
    assert same_bits(one, room_refs(scene_dir, "direct_lighting", 0)[1][0])


def test_a_query_sees_the_moved_mesh(tmp_path):
    # a set without equal-distance ties: the refitted tree and a fresh one give the same bits
    path = _lbvh_sets.write_set(str(tmp_path), "tri257", _lbvh_sets.separated_triangles(257))
    s = sp.Scene.from_file(path)
    s.upload(device=0)
    u, v = np.meshgrid(np.linspace(-1.0, 1.0, 24, dtype=F), np.linspace(-1.0, 1.0, 16, dtype=F))
    o = np.tile(np.array([0.0, 0.0, 3.2], dtype=F), (u.size, 1))
    d = np.stack([u.ravel(), v.ravel(), np.zeros(u.size, dtype=F)], axis=1) - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    seeds = np.arange(u.size) * 2654435761
    still, _ = s.radiance(o, d, seeds, "direct_lighting", 3)
    verts, faces = R.mesh_of(s)
    moved = R.shift(verts, faces)
    assert s.update_mesh(moved, stats=True)["refitted"] == 1
    after, ast = s.radiance(o, d, seeds, "direct_lighting", 3)
    fresh = R.moved_scene(s, moved)
    fresh.upload(device=0)
    want, wst = fresh.radiance(o, d, seeds, "direct_lighting", 3)
    assert same_bits(after, want) and counts(ast) == counts(wst)
    assert not same_bits(after, still)


# ---- 7. refusals on a resident scene ---------------------------------------------------------------------

def test_refusals_on_a_resident_scene(scene_dir):
    s, _ = room(scene_dir, 0)
    rays = room_records(0)
    d_rays = as_device(rays)
    out = torch.zeros((128, 3), dtype=torch.float32, device="cuda")
    with pytest.raises(sp.SimplePathError) as e:
        s.radiance(*fields(rays), "mandelbrot", 2)
    assert e.value.code == _abi.SP_ERR_UNSUPPORTED
    with pytest.raises(sp.SimplePathError) as e:
        s.radiance_device(d_rays.data_ptr() + 8, 64, out.data_ptr(), "direct_lighting", 2)
    assert e.value.code == _abi.SP_ERR_ARG
    q = s._radiance_query("direct_lighting", 2, 128, d_rays.data_ptr())
    q.flags = 4
    assert sp.lib().sp_scene_radiance_rays(s.handle, C.byref(q), out.data_ptr(), None) == _abi.SP_ERR_ARG
    with pytest.raises(sp.SimplePathError) as e:
        s.radiance_device(d_rays.data_ptr(), 128, out.data_ptr(), "direct_lighting", 0)
    assert e.value.code == _abi.SP_ERR_ARG
    with pytest.raises(sp.SimplePathError) as e:
        s.radiance(*fields(rays), "whitted", 2, waves_per_simd=3)
    assert e.value.code == _abi.SP_ERR_ARG
    # more queue items than the int32 queue head counts: refused before anything is touched
    with pytest.raises(sp.SimplePathError) as e:
        s.radiance_device(d_rays.data_ptr(), 64 * (2 ** 31 - 1) + 1, out.data_ptr(), "direct_lighting", 1)
    assert e.value.code == _abi.SP_ERR_UNSUPPORTED
    assert np.all(out.cpu().numpy() == 0.0)  # none of them wrote anything
    # no rays: succeeds, launches nothing
    st = s.radiance_device(0, 0, out.data_ptr(), "direct_lighting", 2)
    assert counts(st) == (0, 0, 0, 0) and st.launches == 0
    empty, st = s.radiance(np.zeros((0, 3)), np.zeros((0, 3)), [], "direct_lighting", 2)
    assert empty.shape == (0, 3) and st.launches == 0
