"""The relight surface of the C ABI (include/simplepath_hip.h, SP_HAS_RELIGHT) without a device:
the header's announcement, struct layouts against the compiler, ctypes and numpy, the refusal order
of sp_scene_set_materials / sp_scene_set_lights / sp_scene_set_env_image on a scene that is not
resident (each returns its code and changes nothing), edits of such a scene showing in desc(), and
the host half of the table check (sp_scene_env_build_check).  One test at the end needs the device:
a scene edited before its upload renders the oracle's image of desc()."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import simplepath_amd as sp
from simplepath_amd import _abi, scenes
from tests import _oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "simplepath_hip.h")
ARG, STATE, OK = _abi.SP_ERR_ARG, _abi.SP_ERR_STATE, _abi.SP_OK

ENV_UPDATE = ("struct_size", "image", "width", "height", "pixels", "d_pixels", "max_radiance", "reserved0", "light_to_world",
              "world_to_light", "reserved")
ENV_STATS = ("struct_size", "rebuilt", "guided", "reserved", "ms_upload", "ms_clamp", "ms_func", "ms_rows", "ms_marginal",
             "ms_guides", "ms_total", "reserved2", "scratch_bytes")
ENV_CHECK = ("struct_size", "builder", "width", "height", "nu", "nv", "guided", "cond_bits", "marg_bits", "marg_int_bits",
             "mismatches", "first_table", "reserved", "first_index", "hash")
NEW = ("sp_scene_set_materials", "sp_scene_set_lights", "sp_scene_set_env_image", "sp_scene_env_check", "sp_scene_env_build_check")


def test_header_announces_the_surface():
    text = open(HEADER).read()
    assert re.search(r"^#define SP_HAS_RELIGHT 1\b", text, re.M)
    assert re.search(r"#define SP_ABI_VERSION 6\b", text)  # new entry points only
    for name in NEW:
        assert name in _abi.SIGNATURES and hasattr(sp.lib(), name), name
    for name in ("set_materials", "set_lights", "set_env_image", "env_check", "env_build_check"):
        assert hasattr(sp.Scene, name), name


def test_struct_layouts_match_the_compiler(tmp_path):
    line = lambda t, fs: ('  printf("%zu' + " %zu" * len(fs) + '\\n", sizeof(' + t + ")"
                          + "".join(f", offsetof({t}, {f})" for f in fs) + ");\n")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "simplepath_hip.h"\nint main(void) {\n'
                   + line("sp_env_update", ENV_UPDATE) + line("sp_env_stats", ENV_STATS) + line("sp_env_check", ENV_CHECK)
                   + "  return SP_HAS_RELIGHT - 1;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, timeout=120)
    rows = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.splitlines()
    types = ((_abi.sp_env_update, ENV_UPDATE), (_abi.sp_env_stats, ENV_STATS), (_abi.sp_env_check, ENV_CHECK))
    for got, (T, fs) in zip(rows, types):
        assert tuple(n for n, _ in T._fields_) == fs
        assert [int(x) for x in got.split()] == [C.sizeof(T)] + [getattr(T, f).offset for f in fs], T
        if T is _abi.sp_env_update:
            continue  # (pointers: numpy has no dtype for them)
        # numpy reads the same layout from the ctypes type
        dt = np.dtype(T)
        assert dt.itemsize == C.sizeof(T) and [dt.fields[f][1] for f in fs] == [getattr(T, f).offset for f in fs]
    assert (C.sizeof(_abi.sp_env_update), C.sizeof(_abi.sp_env_stats), C.sizeof(_abi.sp_env_check)) == (128, 56, 144)


# ---------------------------------------------------------------- helpers
def ibl(scene_dir):
    return sp.Scene.from_file(os.path.join(scene_dir, "material_spheres_ibl.sp"))


def materials_of(scene):
    d = scene.desc()
    return [_abi.sp_material_desc.from_buffer_copy(d.materials[i]) for i in range(d.info.num_materials)]


def lights_of(scene):
    d = scene.desc()
    return [_abi.sp_light_desc.from_buffer_copy(d.lights[i]) for i in range(d.info.num_lights)]


def env_of(scene, image=0):
    e = scene.desc().env_images[image]
    return e, np.ctypeslib.as_array(e.pixels, shape=(e.height, e.width, 3)).copy()


def snapshot(scene):
    """every byte an edit could touch, as the descriptor shows it"""
    d = scene.desc()
    out = [bytes(m) for m in materials_of(scene)] + [bytes(l) for l in lights_of(scene)]
    for i in range(d.num_env_images):
        e, px = env_of(scene, i)
        out += [px.tobytes(), bytes(e.light_to_world), bytes(e.world_to_light), np.float32(e.max_radiance).tobytes()]
    return out


def env_update(scene, px=None, **kw):
    e = scene.desc().env_images[0]
    u = _abi.sp_env_update()
    u.struct_size = C.sizeof(_abi.sp_env_update)
    u.max_radiance = e.max_radiance
    u.light_to_world, u.world_to_light = e.light_to_world, e.world_to_light
    if px is not None:
        u.height, u.width = px.shape[0], px.shape[1]
        u.pixels = px.ctypes.data_as(C.POINTER(C.c_float))
    for k, v in kw.items():
        setattr(u, k, v)
    return u


# ---------------------------------------------------------------- refusals
def test_set_materials_refusals(scene_dir):
    L, scene = sp.lib(), ibl(scene_dir)
    mats = materials_of(scene)
    n = len(mats)
    before = snapshot(scene)
    arr = lambda ms: (_abi.sp_material_desc * len(ms))(*ms)
    good = arr(mats)
    assert L.sp_scene_set_materials(None, good, n) == ARG
    assert L.sp_scene_set_materials(scene.handle, None, n) == ARG
    for count in (n - 1, n + 1, 0, -1):
        assert L.sp_scene_set_materials(scene.handle, good, count) == ARG
    coat = next(i for i, m in enumerate(mats) if m.kind == _abi_kind("clearcoat"))
    for field, value in (("kind", 3), ("kind", -1)):
        bad = materials_of(scene)
        setattr(bad[0], field, value)
        assert L.sp_scene_set_materials(scene.handle, arr(bad), n) == ARG
    for base in (-1, n, n + 7):
        bad = materials_of(scene)
        bad[coat].base = base
        assert L.sp_scene_set_materials(scene.handle, arr(bad), n) == ARG
    bad = materials_of(scene)
    bad[coat].base = coat  # a clearcoat over a clearcoat: what the upload refuses too
    assert L.sp_scene_set_materials(scene.handle, arr(bad), n) == _abi.SP_ERR_UNSUPPORTED
    # the order: the count is judged before the materials
    bad = materials_of(scene)
    bad[0].kind = 9
    assert L.sp_scene_set_materials(scene.handle, arr(bad), n + 1) == ARG and "num_materials" in L.sp_last_error().decode()
    assert snapshot(scene) == before
    assert L.sp_scene_set_materials(scene.handle, good, n) == OK and snapshot(scene) == before


def _abi_kind(name):
    return {"lambertian": 0, "glossy": 1, "clearcoat": 2}[name]


def test_set_lights_refusals(scene_dir):
    L, scene = sp.lib(), ibl(scene_dir)
    lights = lights_of(scene)
    assert [l.kind for l in lights] == [2]
    before = snapshot(scene)
    arr = lambda ls: (_abi.sp_light_desc * max(len(ls), 1))(*ls)
    assert L.sp_scene_set_lights(None, arr(lights), 1) == ARG
    assert L.sp_scene_set_lights(scene.handle, arr(lights), -1) == ARG
    assert L.sp_scene_set_lights(scene.handle, None, 1) == ARG
    for kind in (-1, 3):
        bad = lights_of(scene)
        bad[0].kind = kind
        assert L.sp_scene_set_lights(scene.handle, arr(bad), 1) == ARG
    for image in (-1, 1, 5):
        bad = lights_of(scene)
        bad[0].image = image
        assert L.sp_scene_set_lights(scene.handle, arr(bad), 1) == ARG
    assert snapshot(scene) == before
    # a scene without env images accepts no image light
    bunny = sp.Scene.from_file(os.path.join(scene_dir, "bunny.sp"))
    assert bunny.desc().num_env_images == 0
    assert L.sp_scene_set_lights(bunny.handle, arr(lights), 1) == ARG
    assert L.sp_scene_set_lights(scene.handle, arr(lights), 1) == OK and snapshot(scene) == before


def test_set_env_image_refusals(scene_dir):
    L, scene = sp.lib(), ibl(scene_dir)
    e, px = env_of(scene)
    before = snapshot(scene)
    st = _abi.sp_env_stats()
    st.struct_size = C.sizeof(_abi.sp_env_stats)
    bad_stats = _abi.sp_env_stats()
    bad_stats.struct_size = 52
    small = np.ones((3, 5, 3), dtype=np.float32)
    fake = C.c_void_p(4096)  # never dereferenced: each call below is refused before it
    bad = [env_update(scene, px, struct_size=0), env_update(scene, px, struct_size=C.sizeof(_abi.sp_env_update) + 8),
           env_update(scene, px, reserved0=1), env_update(scene, px, reserved=(C.c_int32 * 4)(0, 0, 0, 1)),
           env_update(scene, px, image=-1), env_update(scene, px, image=2),
           env_update(scene, px, d_pixels=fake),
           env_update(scene, px, width=0), env_update(scene, px, height=0), env_update(scene, px, width=-4),
           env_update(scene, px, width=40000),
           env_update(scene, None, image=1),               # an append without pixels
           env_update(scene, None, width=5, height=3),     # no pixels, another size
           env_update(scene, None, width=e.width)]         # no pixels, half a size
    for u in bad:
        assert L.sp_scene_set_env_image(scene.handle, C.byref(u), C.byref(st)) == ARG, L.sp_last_error()
        assert L.sp_scene_set_env_image(scene.handle, C.byref(u), None) == ARG
        assert snapshot(scene) == before
    good = env_update(scene, small)
    assert L.sp_scene_set_env_image(None, C.byref(good), None) == ARG
    assert L.sp_scene_set_env_image(scene.handle, None, None) == ARG
    assert L.sp_scene_set_env_image(scene.handle, C.byref(good), C.byref(bad_stats)) == ARG
    # the order: struct size before reserved before image before the pointers before the size
    u = env_update(scene, px, struct_size=4, reserved0=1, image=9, d_pixels=fake, width=0)
    for fix, word in ((dict(struct_size=C.sizeof(_abi.sp_env_update)), "struct_size"), (dict(reserved0=0), "reserved"),
                      (dict(image=0), "image"), (dict(d_pixels=None), "both"), (dict(width=e.width), "size")):
        assert L.sp_scene_set_env_image(scene.handle, C.byref(u), None) == ARG and word in L.sp_last_error().decode()
        for k, v in fix.items():
            setattr(u, k, v)
    # device pixels need a resident scene: the last refusal
    u = env_update(scene, None, d_pixels=fake, width=5, height=3)
    assert L.sp_scene_set_env_image(scene.handle, C.byref(u), None) == STATE
    assert snapshot(scene) == before
    # the checks' own refusals
    c = _abi.sp_env_check()
    c.struct_size = C.sizeof(_abi.sp_env_check)
    assert L.sp_scene_env_build_check(scene.handle, 1, C.byref(c)) == ARG
    assert L.sp_scene_env_build_check(scene.handle, -1, C.byref(c)) == ARG
    assert L.sp_scene_env_build_check(None, 0, C.byref(c)) == ARG and L.sp_scene_env_build_check(scene.handle, 0, None) == ARG
    assert L.sp_scene_env_check(scene.handle, 0, C.byref(c)) == STATE
    c.struct_size = 8
    assert L.sp_scene_env_build_check(scene.handle, 0, C.byref(c)) == ARG and L.sp_scene_env_check(scene.handle, 0, C.byref(c)) == ARG


# ---------------------------------------------------------------- edits of a scene that is not resident
def edit_everything(scene):
    mats = materials_of(scene)
    for m in mats:
        if m.kind == 0:
            m.kind, m.alpha_x, m.alpha_y, m.microfacet_ior = 1, 0.25, 0.125, 1.7
            m.microfacet_r = (C.c_float * 3)(1.0, 1.0, 1.0)
        m.lambert_albedo = (C.c_float * 3)(0.2, 0.1, 0.05)
    scene.set_materials(mats)
    sky = scenes.night_sky_image(20, 10, seed=5)
    stats = scene.set_env_image(0, pixels=sky, max_radiance=3.0, light_to_world=[[0, 0, 1], [0, 1, 0], [-1, 0, 0]], stats=True)
    assert stats["rebuilt"] == 0 and stats["scratch_bytes"] == 0
    return mats, sky


def test_non_resident_edits_show_in_desc(scene_dir):
    scene = ibl(scene_dir)
    mats, sky = edit_everything(scene)
    assert [bytes(m) for m in materials_of(scene)] == [bytes(m) for m in mats]
    e, px = env_of(scene)
    assert (e.width, e.height, e.max_radiance) == (20, 10, 3.0) and np.array_equal(px.view(np.uint32), sky.view(np.uint32))
    assert list(e.light_to_world.vx) == [0, 0, 1] and list(e.world_to_light.vx) == [0, 0, -1]
    # an appended image, then a light list that names it beside a sphere light taken from another scene
    scene.set_env_image(1, pixels=np.full((2, 4, 3), 0.5, dtype=np.float32))
    assert scene.desc().num_env_images == 2
    lamp = lights_of(sp.Scene.from_file(os.path.join(scene_dir, "material_spheres.sp")))
    new = lights_of(scene)
    new[0].image = 1
    scene.set_lights(new + [l for l in lamp if l.kind == 0])
    got = lights_of(scene)
    assert scene.info().num_lights == len(got) == 1 + sum(l.kind == 0 for l in lamp) and got[0].image == 1
    scene.set_lights([])
    assert scene.info().num_lights == 0


# ---------------------------------------------------------------- the host half of the table check
def test_env_build_check(scene_dir):
    scene = ibl(scene_dir)
    e, px = env_of(scene)
    a = scene.env_build_check(0)
    assert (a["width"], a["height"], a["nu"], a["nv"]) == (96, 48, 192, 96) and a["builder"] == "host"
    assert a["guided"] == 1 and a["mismatches"] == 0 and (a["cond_bits"], a["marg_bits"]) == (8, 7)
    assert all(a["hashes"][t] != 0 for t in _abi.ENV_TABLES)
    # a transform-only edit changes no table
    scene.set_env_image(0, light_to_world=[[0, 1, 0], [-1, 0, 0], [0, 0, 1]])
    assert scene.env_build_check(0) == a
    # one texel changes the hashes of what depends on it
    px2 = px.copy()
    px2[10, 17] = (7.0, 8.0, 9.0)
    scene.set_env_image(0, pixels=px2)
    b = scene.env_build_check(0)
    for t in ("radiance", "cond_func", "cond_cdf", "cond_int", "marg_func", "marg_cdf"):
        assert b["hashes"][t] != a["hashes"][t], t
    assert b["marg_int_bits"] != a["marg_int_bits"]
    scene.set_env_image(0, pixels=px)
    assert scene.env_build_check(0) == a
    # a NaN texel: some row is not ordered, the map has no guides
    px2 = px.copy()
    px2[20, 40, 1] = np.nan
    scene.set_env_image(0, pixels=px2)
    c = scene.env_build_check(0)
    assert c["guided"] == 0 and c["hashes"]["cond_guide"] == 0 and c["hashes"]["marg_guide"] == 0


# ---------------------------------------------------------------- and its upload (the one test here that needs the device)
@pytest.mark.gpu
def test_upload_after_non_resident_edits_renders_the_oracle(scene_dir):
    scene = ibl(scene_dir)
    scene.set_resolution(24, 16)
    edit_everything(scene)
    scene.upload(device=0, bvh_mode=1)
    assert scene.env_check(0)["mismatches"] == 0
    for integrator, spp in (("direct_lighting", 3), ("iterative_rrnee", 2)):
        g, st = sp.render_tiles(scene, integrator, spp)
        c, cst = _oracle.render(scene, sp.string_to_integrator_type(integrator), spp, variant="spm")
        assert (st.rays, st.shadow_rays, st.samples) == (cst["rays"], cst["shadow_rays"], cst["samples"])
        assert np.array_equal(g.view(np.uint32), c.view(np.uint32)), integrator
