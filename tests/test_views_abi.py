"""sp_render_views without a device (include/simplepath_hip.h, "many views in one launch"): the
announcement in the header, the layout of sp_view_params in C and ctypes, and every refusal in the
order the header states, on a scene that is not resident -- so the residency check, which comes last
of them, answers only once everything before it is in order."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import simplepath_amd as sp
from simplepath_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "simplepath_hip.h")
ARG, STATE = _abi.SP_ERR_ARG, _abi.SP_ERR_STATE
ALIGNED, ODD = 0x1000, 0x1008  # stand-in device addresses: validation never reads through them
FIELDS = ("integrator", "samples_per_pixel", "num_views", "cameras", "d_cameras", "tile_ids", "d_tile_ids", "num_tiles",
          "stream", "waves_per_simd", "flags", "reserved")


def test_header_announces_the_surface():
    src = open(HEADER).read()
    assert re.search(r"^#define SP_HAS_VIEWS 1\b", src, re.M)
    assert re.search(r"#define SP_ABI_VERSION 6\b", src)  # new entry points only
    for name in ("sp_render_views", "sp_render_views_host"):
        assert re.search(r"\b%s\(" % name, src), name
        assert name in _abi.SIGNATURES and hasattr(sp.lib(), name), name
    for name in ("render_views", "render_views_device"):
        assert name in sp.__all__
    # what the views share, stated where a caller reads it
    assert "SAME random" in src and "correlated" in src


def test_struct_layout_matches_the_compiler(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "simplepath_hip.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(sp_view_params));\n'
                   + "".join('  printf(" %%zu", offsetof(sp_view_params, %s));\n' % f for f in FIELDS)
                   + '  printf("\\n%zu %zu\\n", sizeof(sp_camera_desc), offsetof(sp_camera_desc, film_width));\n'
                   "  return SP_HAS_VIEWS == 1 && SP_HAS_CAMERA_EDIT == 1 ? 0 : 1;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, timeout=120)
    a, b = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.splitlines()
    V = _abi.sp_view_params
    assert [name for name, _ in V._fields_] == ["struct_size", *FIELDS]
    assert [int(x) for x in a.split()] == [C.sizeof(V)] + [getattr(V, f).offset for f in FIELDS] \
        == [88, 4, 8, 12, 16, 24, 32, 40, 48, 56, 64, 68, 72]
    assert [int(x) for x in b.split()] == [C.sizeof(_abi.sp_camera_desc), _abi.sp_camera_desc.film_width.offset] == [56, 48]


@pytest.fixture(scope="module")
def scene(scene_dir):
    s = sp.Scene.from_file(os.path.join(scene_dir, "bunny.sp"))  # never uploaded
    s.set_resolution(20, 12)  # 3 x 2 tiles
    return s


def params(scene, views=2, host=True, d_cameras=0, tiles=None, d_tiles=0, n_tiles=0, spp=4, flags=0):
    p = _abi.sp_view_params()
    p.struct_size = C.sizeof(p)
    p.integrator, p.samples_per_pixel, p.num_views, p.flags = _abi.INTEGRATORS["direct_lighting"], spp, views, flags
    keep = [None, None]
    if host:
        keep[0] = (_abi.sp_camera_desc * max(views, 1))(*[scene.desc().camera] * max(views, 1))
        p.cameras = C.cast(keep[0], C.POINTER(_abi.sp_camera_desc))
    p.d_cameras = d_cameras or None
    if tiles is not None:
        keep[1] = np.asarray(tiles, dtype=np.int32)
        p.tile_ids = keep[1].ctypes.data_as(C.POINTER(C.c_int32))
        p.num_tiles = keep[1].size
    if d_tiles:
        p.d_tile_ids, p.num_tiles = d_tiles, n_tiles
    p._keep = keep
    return p


def test_refusals_come_in_the_stated_order(scene):
    L = sp.lib()
    OUT = C.c_void_p(ALIGNED)
    call = lambda s, p, out=OUT: L.sp_render_views(s, None if p is None else C.byref(p), out, None)
    err = lambda: L.sp_last_error()
    # everything in order: only the residency is missing
    assert call(scene.handle, params(scene)) == STATE and b"sp_scene_upload" in err()
    assert call(scene.handle, params(scene, host=False, d_cameras=ALIGNED)) == STATE
    assert call(scene.handle, params(scene, tiles=[5, 0, 3])) == STATE
    assert call(scene.handle, params(scene, d_tiles=ALIGNED, n_tiles=3, flags=sp.PER_LANE_QUERIES)) == STATE
    # 1. null scene, params (or output) -- before anything in the params is looked at
    bad = params(scene)
    bad.struct_size = 0
    assert call(None, bad) == ARG and b"null" in err()
    assert call(scene.handle, None) == ARG and b"null" in err()
    assert call(scene.handle, params(scene), None) == ARG and b"null" in err()
    # 2. struct_size and reserved words -- before the flags
    p = params(scene, flags=1)
    p.struct_size -= 8
    assert call(scene.handle, p) == ARG and b"struct_size" in err()
    for k in range(4):
        p = params(scene, flags=1)
        p.reserved[k] = 1
        assert call(scene.handle, p) == ARG and b"reserved" in err()
    # 3. flags -- before the view count
    for flags in (1, 2, 3, 4, 16, sp.PER_LANE_QUERIES | 1, -1):
        assert call(scene.handle, params(scene, views=0, flags=flags)) == ARG and b"flags" in err()
    # 4. num_views < 1 -- before the camera pointers
    for views in (0, -1):
        assert call(scene.handle, params(scene, views=views, host=False)) == ARG and b"num_views" in err()
    # 5. exactly one of cameras / d_cameras, the device one aligned -- before the cameras are read
    assert call(scene.handle, params(scene, host=False)) == ARG and b"cameras" in err()
    assert call(scene.handle, params(scene, host=True, d_cameras=ALIGNED)) == ARG and b"cameras" in err()
    assert call(scene.handle, params(scene, host=False, d_cameras=ODD, tiles=[9])) == ARG and b"aligned" in err()
    # 6. a host camera with another film size or a non-finite value -- before the tile list
    for edit in ("w", "h", "nan", "inf"):
        p = params(scene, tiles=[9])
        cam = p._keep[0][1]
        if edit == "w":
            cam.film_width += 1
        elif edit == "h":
            cam.film_height -= 1
        else:
            cam.transform.vz[1] = math.nan if edit == "nan" else math.inf
        assert call(scene.handle, p) == ARG and (b"film size" if edit in "wh" else b"finite") in err(), edit
    # 7. the tile-list rules of sp_render_tiles -- before the sample count
    p = params(scene, tiles=[1], d_tiles=ALIGNED, n_tiles=1, spp=0)
    assert call(scene.handle, p) == ARG and b"not both" in err()
    assert call(scene.handle, params(scene, d_tiles=ALIGNED, n_tiles=-1, spp=0)) == ARG and b"num_tiles" in err()
    for tiles in ([6], [-1], [0, 1, 99]):
        assert call(scene.handle, params(scene, tiles=tiles, spp=0)) == ARG and b"out of range" in err()
    # 8. samples_per_pixel == 0 -- before the residency
    assert call(scene.handle, params(scene, spp=0)) == ARG and b"samples_per_pixel" in err()
    # 9. SP_ERR_STATE is last of them: nothing above was wrong with the first calls


def test_the_host_variant_and_the_wrappers_refuse_alike(scene):
    L = sp.lib()
    out = np.zeros((2 * 6, 64, 3), dtype=np.float32)
    host = lambda s, p, o=out: L.sp_render_views_host(s, None if p is None else C.byref(p),
                                                       None if o is None else o.ctypes.data_as(C.POINTER(C.c_float)), None)
    assert host(None, params(scene)) == ARG
    assert host(scene.handle, None) == ARG
    assert host(scene.handle, params(scene), None) == ARG
    assert host(scene.handle, params(scene, views=0)) == ARG
    assert host(scene.handle, params(scene, tiles=[7])) == ARG
    assert host(scene.handle, params(scene, spp=0)) == ARG
    assert host(scene.handle, params(scene)) == STATE
    cam = scene.desc().camera
    with pytest.raises(sp.SimplePathError) as e:
        sp.render_views(scene, "direct_lighting", 2, [cam, cam])
    assert e.value.code == STATE
    with pytest.raises(sp.SimplePathError) as e:
        sp.render_views(scene, "direct_lighting", 2, [])
    assert e.value.code == ARG
    with pytest.raises(sp.SimplePathError) as e:
        sp.render_views_device(scene, "direct_lighting", 2, None, None, ALIGNED, d_cameras=ODD, num_views=2)
    assert e.value.code == ARG
    with pytest.raises(sp.SimplePathError) as e:
        sp.render_views_device(scene, "direct_lighting", 2, [cam], [0, 1], ALIGNED, stats=False)
    assert e.value.code == STATE
