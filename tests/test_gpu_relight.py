"""Relighting a resident scene on the GPU (Scene.set_materials / set_lights / set_env_image).

The contract is refit's: an edited resident scene is, in every bit, what a fresh upload of the
edited descriptor would be.  So after every edit
  * a scene resident with bvh_mode=1 renders the oracle's image of scene.desc(), with equal ray,
    shadow-ray and sample counts, for DirectLighting and IterativeRRNEE;
  * a scene resident with bvh_mode=0 renders the image and all four counts (draws too) of a fresh
    Scene.from_desc(scene.desc()) uploaded with the same options, and holds as many device bytes.
Small frames, 2-3 samples per pixel.  Then the other calls on the scene (ray query, radiance query,
render_views), progress objects, work queued ahead of an edit, and null edits."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import simplepath_amd as sp
from simplepath_amd import _abi, scenes
from tests import _oracle

pytestmark = pytest.mark.gpu

INTEGRATORS = (("direct_lighting", 3), ("iterative_rrnee", 2))
WALKS = {"stack": dict(), "stackless": dict(stackless=True), "stack_max_1": dict(stack_max_levels=1)}


# ---------------------------------------------------------------- helpers
def load(scene_dir, name, w, h, **upload_options):
    s = sp.Scene.from_file(os.path.join(scene_dir, name))
    s.set_resolution(w, h)
    s.upload(device=0, **upload_options)
    return s


def materials_of(scene):
    d = scene.desc()
    return [_abi.sp_material_desc.from_buffer_copy(d.materials[i]) for i in range(d.info.num_materials)]


def lights_of(scene):
    d = scene.desc()
    return [_abi.sp_light_desc.from_buffer_copy(d.lights[i]) for i in range(d.info.num_lights)]


def f3(*v):
    return (C.c_float * 3)(*[float(x) for x in v])


def sphere_light(center, radius, radiance):
    """a sphere_light's descriptor: object_to_world = translate * scale, its inverse, its normal matrix"""
    l = _abi.sp_light_desc()
    l.kind, l.image = 0, -1
    l.radiance = f3(*radiance)
    s, i = float(np.float32(radius)), float(np.float32(1.0) / np.float32(radius))
    for m, d in ((l.object_to_world, s), (l.world_to_object, i), (l.normal_to_world, i)):
        m.vx, m.vy, m.vz = f3(d, 0, 0), f3(0, d, 0), f3(0, 0, d)
    l.object_to_world.p = f3(*center)
    l.world_to_object.p = f3(*[-float(np.float32(c)) * i for c in center])
    return l


def edited_materials(scene):
    """every material changed: lambertian to glossy, other alphas, clearcoat colour and IOR"""
    mats = materials_of(scene)
    for k, m in enumerate(mats):
        if m.kind == 0:
            m.kind, m.microfacet_ior, m.sample_visible_area = 1, 1.6, 1
            m.microfacet_r = f3(1, 1, 1)
            m.alpha_x, m.alpha_y = 0.3, 0.2
            m.lambert_albedo = f3(0.25, 0.1 + 0.02 * k, 0.05)
        elif m.kind == 1:
            m.alpha_x, m.alpha_y = 0.15 + 0.05 * k, 0.4
            m.lambert_albedo = f3(0.05, 0.2, 0.1 + 0.02 * k)
        else:
            m.coat_ior = 1.3 + 0.05 * k
            m.coat_color = f3(0.9, 0.6, 0.3)
    return mats


def oracle_of(scene, integrator, spp):
    return _oracle.render(scene, sp.string_to_integrator_type(integrator), spp, variant="spm")


def equals_oracle(scene, what, integrators=INTEGRATORS):
    for integrator, spp in integrators:
        g, st = sp.render_tiles(scene, integrator, spp)
        c, cst = oracle_of(scene, integrator, spp)
        assert (st.rays, st.shadow_rays, st.samples) == (cst["rays"], cst["shadow_rays"], cst["samples"]), (what, integrator)
        bad = np.argwhere(np.any(g.view(np.uint32) != c.view(np.uint32), axis=-1))
        assert bad.size == 0, (what, integrator, bad[:6].tolist())


def equals_fresh(scene, what, upload_options, integrators=INTEGRATORS):
    fresh = sp.Scene.from_desc(scene.desc())
    fresh.upload(device=0, **upload_options)
    assert scene.device_bytes() == fresh.device_bytes(), what
    for integrator, spp in integrators:
        g, st = sp.render_tiles(scene, integrator, spp)
        f, fst = sp.render_tiles(fresh, integrator, spp)
        counts = lambda s: (s.rays, s.shadow_rays, s.samples, s.rng_draws, s.stack_depth)
        assert counts(st) == counts(fst), (what, integrator, counts(st), counts(fst))
        assert np.array_equal(g.view(np.uint32), f.view(np.uint32)), (what, integrator)
    return fresh


def pair(scene_dir, name, w, h, **options):
    """the scene resident twice: in the reference order (against the oracle) and as a SAH upload (against a fresh one)"""
    return load(scene_dir, name, w, h, bvh_mode=1, **options), load(scene_dir, name, w, h, bvh_mode=0, **options)


# ---------------------------------------------------------------- materials
@pytest.mark.parametrize("name,w,h", [("closed_room.sp", 16, 8), ("material_spheres.sp", 24, 16)])
def test_material_edits(scene_dir, name, w, h):
    ref, sah = pair(scene_dir, name, w, h)
    before = sp.render_tiles(ref, "direct_lighting", 2)[0]
    for s in (ref, sah):
        nbytes = s.device_bytes()
        s.set_materials(edited_materials(s))
        assert s.device_bytes() == nbytes
    assert not np.array_equal(before, sp.render_tiles(ref, "direct_lighting", 2)[0])  # the edit is seen
    equals_oracle(ref, name)
    equals_fresh(sah, name, dict(bvh_mode=0))


# ---------------------------------------------------------------- lights
def light_edits(scene):
    """(name, light list) one after another, from material_spheres.sp's constant
    environment + one sphere light, with env image 0 appended to the scene"""
    base = lights_of(scene)
    env = [l for l in base if l.kind == 1]
    lamp = [l for l in base if l.kind == 0]
    assert len(env) == 1 and len(lamp) == 1
    moved = sphere_light((2.0, 5.0, 4.0), 0.75, lamp[0].radiance)
    bright = sphere_light((2.0, 5.0, 4.0), 0.75, (35.0, 30.0, 12.0))
    more = [bright, sphere_light((-4.0, 3.0, 5.0), 0.5, (10.0, 20.0, 30.0)), sphere_light((0.5, -2.0, 7.0), 0.25, (50.0, 50.0, 50.0))]
    sky = _abi.sp_light_desc.from_buffer_copy(env[0])
    sky.kind, sky.image = 2, 0
    # the reference-order light BVH keeps up to four lights in one leaf: three lights are still a leaf, six get inner nodes
    six = more + [sphere_light((-3.0 + 2.5 * k, 6.0, 2.0 + k), 0.25, (8.0 + k, 6.0, 4.0)) for k in range(3)]
    return [("move_scale", env + [moved]), ("radiance", env + [bright]), ("three_lights", [more[1]] + env + [more[0], more[2]]),
            ("six_lights", six[:4] + env + six[4:]), ("no_sphere_lights", env), ("image_light", [sky] + more[:2]), ("back", base)]


@pytest.mark.parametrize("walk", list(WALKS))
def test_light_edits(scene_dir, walk):
    options = WALKS[walk]
    ref, sah = pair(scene_dir, "material_spheres.sp", 24, 16, **options)
    sky = scenes.night_sky_image(20, 10, seed=8)
    first = {}
    for s in (ref, sah):
        assert s.desc().num_env_images == 0
        s.set_env_image(0, pixels=sky, max_radiance=50.0)  # appended; no light names it yet
        assert s.desc().num_env_images == 1 and s.env_check(0)["mismatches"] == 0
        first[s] = sp.render_tiles(s, "direct_lighting", 2)
    depths = []
    for name, lights in light_edits(ref):
        what = (walk, name)
        for s in (ref, sah):
            s.set_lights(lights)
            assert [bytes(l) for l in lights_of(s)] == [bytes(l) for l in lights], what
        depths.append(ref.bvh_build_info(1)["light_depth"])
        equals_oracle(ref, what)
        equals_fresh(sah, what, dict(bvh_mode=0, **options))
        equals_fresh(ref, what, dict(bvh_mode=1, **options), integrators=INTEGRATORS[:1])
    # the light BVH follows the list: one light, one, three (one leaf still), six (inner nodes), none, two, one
    assert depths[0] == depths[1] == depths[2] == depths[5] == depths[6] == 1 and depths[3] > 1 and depths[4] == 0, depths
    for s in (ref, sah):  # back at the first list: the first image and counts
        g, st = sp.render_tiles(s, "direct_lighting", 2)
        assert np.array_equal(g.view(np.uint32), first[s][0].view(np.uint32)) and st.rng_draws == first[s][1].rng_draws


# ---------------------------------------------------------------- sky
ROT = [[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]]


@pytest.mark.parametrize("replay", [False, True], ids=["guides", "env_replay"])
def test_sky_edits(scene_dir, replay):
    options = dict(env_replay=replay)
    ref, sah = pair(scene_dir, "material_spheres_ibl.sp", 24, 16, **options)
    edits = [("swap_67x33", dict(pixels=scenes.night_sky_image(67, 33, seed=4))), ("max_radiance_3", dict(max_radiance=3.0)),
             ("rotate", dict(light_to_world=ROT))]
    last = None
    for name, edit in edits:
        what = (replay, name)
        for s in (ref, sah):
            st = s.set_env_image(0, stats=True, **edit)
            assert st["rebuilt"] == (0 if name == "rotate" else 1), what
            assert s.env_check(0)["mismatches"] == 0, what
        equals_oracle(ref, what)
        equals_fresh(sah, what, dict(bvh_mode=0, **options))
        g = sp.render_tiles(ref, "direct_lighting", 2)[0]
        assert last is None or not np.array_equal(g, last), what  # every edit is seen
        last = g


def test_sky_appended_to_a_scene_without_one(scene_dir):
    ref, sah = pair(scene_dir, "bunny_scan.sp", 32, 24)
    sky = scenes.night_sky_image(40, 20, seed=12)
    for s in (ref, sah):
        assert s.desc().num_env_images == 0
        nbytes = s.device_bytes()
        st = s.set_env_image(0, pixels=sky, max_radiance=20.0, light_to_world=ROT, stats=True)
        assert st["rebuilt"] == 1 and s.device_bytes() > nbytes
        light = _abi.sp_light_desc()
        light.kind, light.image = 2, 0
        light.radiance = f3(1, 1, 1)
        s.set_lights(lights_of(s) + [light])
    equals_oracle(ref, "bunny_scan + sky")
    equals_fresh(sah, "bunny_scan + sky", dict(bvh_mode=0))


# ---------------------------------------------------------------- the other calls on the scene
def relit(scene_dir, **options):
    s = load(scene_dir, "material_spheres_ibl.sp", 24, 16, **options)
    s.set_materials(edited_materials(s))
    s.set_env_image(0, pixels=scenes.night_sky_image(67, 33, seed=4), max_radiance=30.0, light_to_world=ROT)
    s.set_lights(lights_of(s) + [sphere_light((3.0, 4.0, 6.0), 0.5, (20.0, 20.0, 20.0))])
    return s


def test_other_calls_after_edits_equal_the_fresh_upload(scene_dir):
    s = relit(scene_dir)
    fresh = equals_fresh(s, "relit", dict(bvh_mode=0))
    rng = np.random.default_rng(5)
    o = np.tile(np.array([[0.0, 0.0, 12.0]], np.float32), (256, 1))
    d = rng.normal(size=(256, 3)).astype(np.float32)
    d[:, 2] = -np.abs(d[:, 2]) - 1.0
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    ha, hb = s.trace(o, d), fresh.trace(o, d)
    assert ha.tobytes() == hb.tobytes() and np.any(ha["kind"] >= 0)
    seeds = np.arange(256, dtype=np.uint32) * 7 + 1
    for integrator, spp in INTEGRATORS:
        ra, sa = s.radiance(o, d, seeds, integrator, spp)
        rb, sb = fresh.radiance(o, d, seeds, integrator, spp)
        assert np.array_equal(ra.view(np.uint32), rb.view(np.uint32)) and (sa.rays, sa.rng_draws) == (sb.rays, sb.rng_draws)
    cams = [sp.camera_look_at((0, 0, 12), (0, 0, 0), (0, 1, 0), 45.0, 24, 16), sp.camera_look_at((6, 2, 10), (0, 0, 0), (0, 1, 0), 50.0, 24, 16)]
    va, vsa = sp.render_views(s, "direct_lighting", 2, cams)
    vb, vsb = sp.render_views(fresh, "direct_lighting", 2, cams)
    assert np.array_equal(va.view(np.uint32), vb.view(np.uint32)) and (vsa.rays, vsa.rng_draws) == (vsb.rays, vsb.rng_draws)


# ---------------------------------------------------------------- progress objects
def test_progress_objects_across_an_edit(scene_dir):
    s = load(scene_dir, "material_spheres_ibl.sp", 24, 16, bvh_mode=1)
    edits = (lambda: s.set_materials(edited_materials(s)),
             lambda: s.set_lights(lights_of(s) + [sphere_light((3.0, 4.0, 6.0), 0.5, (20.0, 20.0, 20.0))]),
             lambda: s.set_env_image(0, max_radiance=7.0),
             lambda: s.set_env_image(0, light_to_world=ROT))
    for edit in edits:
        old = sp.Progressive(s, "direct_lighting")
        old.render(1)
        edit()
        with pytest.raises(_abi.SimplePathError) as err:
            old.render(1)
        assert err.value.code == _abi.SP_ERR_STATE
        old.close()
    new = sp.Progressive(s, "direct_lighting")
    new.render(1)
    g, _ = new.render(2)
    one, _ = sp.render_tiles(s, "direct_lighting", 3)
    assert np.array_equal(g.view(np.uint32), one.view(np.uint32))
    c, _ = oracle_of(s, "direct_lighting", 3)
    assert np.array_equal(g.view(np.uint32), c.view(np.uint32))


# ---------------------------------------------------------------- work queued ahead of an edit
def test_an_edit_waits_for_queued_renders(scene_dir):
    s = load(scene_dir, "material_spheres_ibl.sp", 64, 48, bvh_mode=1)
    tiles = sp.TileScheduler(64, 48).get_num_tiles()
    outs = {i: torch.zeros((tiles, 64, 3), dtype=torch.float32, device="cuda:0") for i, _ in INTEGRATORS}
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    edits = {"direct_lighting": lambda: s.set_env_image(0, pixels=scenes.night_sky_image(67, 33, seed=4), max_radiance=3.0),
             "iterative_rrnee": lambda: (s.set_materials(edited_materials(s)), s.set_lights([sphere_light((3, 4, 6), 0.5, (9, 9, 9))]))}
    expected = {}
    for integrator, spp in INTEGRATORS:
        expected[integrator] = oracle_of(s, integrator, spp)[0]  # of the scene as it is when the render is queued
        sp.render_tiles_device(s, integrator, spp, None, outs[integrator].data_ptr(), stream=stream.cuda_stream, stats=False)
        edits[integrator]()  # issued behind the queued render, which still reads the old arrays
    stream.synchronize()
    torch.cuda.synchronize()
    for integrator, _ in INTEGRATORS:
        assert np.array_equal(outs[integrator].cpu().numpy().view(np.uint32), expected[integrator].view(np.uint32)), integrator
    equals_oracle(s, "after the queued edits")


# ---------------------------------------------------------------- null edits
def test_null_edits_change_nothing(scene_dir):
    for options in (dict(bvh_mode=0), dict(bvh_mode=1, env_replay=True)):
        s = load(scene_dir, "material_spheres_ibl.sp", 24, 16, **options)
        s.set_lights(lights_of(s) + [sphere_light((3.0, 4.0, 6.0), 0.5, (20.0, 20.0, 20.0))])
        nbytes, check = s.device_bytes(), s.env_check(0)
        before = {i: sp.render_tiles(s, i, spp) for i, spp in INTEGRATORS}
        e = s.desc().env_images[0]
        px = np.ctypeslib.as_array(e.pixels, shape=(e.height, e.width, 3)).copy()
        s.set_materials(materials_of(s))
        s.set_lights(lights_of(s))
        assert s.set_env_image(0, pixels=px, stats=True)["rebuilt"] == 1
        assert s.set_env_image(0, stats=True)["rebuilt"] == 0
        after = s.env_check(0)
        assert s.device_bytes() == nbytes and after["mismatches"] == 0 and after["hashes"] == check["hashes"]
        for i, spp in INTEGRATORS:
            g, st = sp.render_tiles(s, i, spp)
            g0, st0 = before[i]
            assert (st.rays, st.shadow_rays, st.samples, st.rng_draws) == (st0.rays, st0.shadow_rays, st0.samples, st0.rng_draws)
            assert np.array_equal(g.view(np.uint32), g0.view(np.uint32))
