"""Camera edits without a device (include/simplepath_hip.h, "camera edits"): the announcement in the
header, sp_camera_look_at against the parser's perspective_camera block bit for bit, its refusals,
and sp_scene_set_camera on a scene that is not resident -- validation order, the descriptor, and
the image size the transform then fixes."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import simplepath_amd as sp
from simplepath_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "simplepath_hip.h")
ARG, STATE = _abi.SP_ERR_ARG, _abi.SP_ERR_STATE

SCENE = """version: 1

scene_parameters {
    output_file_name: "camera.pfm"
    width: %d
    height: %d
}

perspective_camera {
    origin: %s
    look_at: %s
    up: %s
    fov: %s
}

material_lambertian {
    name: "grey"
    diffuse: 0.5 0.5 0.5
}

sphere {
    material: "grey"
}

environment_light {
    radiance: 1.0 1.0 1.0
}
"""

# (eye, look_at, up, fov): values a float holds exactly, so text and ctypes give the same floats
CAMERAS = [((0.0, 0.0, 10.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 45.0),
           ((3.5, 1.25, -6.0), (0.25, 0.5, 0.125), (0.125, 1.0, 0.25), 37.5)]


def bits(cam: _abi.sp_camera_desc) -> np.ndarray:
    t = cam.transform
    return np.array([*t.vx, *t.vy, *t.vz, *t.p], dtype=np.float32).view(np.uint32)


def text(v) -> str:
    return " ".join(repr(float(x)) for x in v)


def test_header_announces_the_surface():
    src = open(HEADER).read()
    assert re.search(r"^#define SP_HAS_CAMERA_EDIT 1\b", src, re.M)
    assert re.search(r"#define SP_ABI_VERSION 6\b", src)  # new entry points only
    for name in ("sp_camera_look_at", "sp_scene_set_camera"):
        assert re.search(r"\b%s\(" % name, src), name
        assert name in _abi.SIGNATURES and hasattr(sp.lib(), name), name
    assert "camera_look_at" in sp.__all__ and hasattr(sp.Scene, "set_camera")
    assert C.sizeof(_abi.sp_camera_desc) == 56 and _abi.sp_camera_desc.film_width.offset == 48


@pytest.mark.parametrize("w,h", [(40, 24), (64, 40)])
@pytest.mark.parametrize("eye,look,up,fov", CAMERAS)
def test_look_at_is_the_parsers_camera(w, h, eye, look, up, fov):
    parsed = sp.Scene.from_string(SCENE % (w, h, text(eye), text(look), text(up), repr(fov))).desc().camera
    made = sp.camera_look_at(eye, look, up, fov, w, h)
    assert (made.film_width, made.film_height) == (parsed.film_width, parsed.film_height) == (w, h)
    assert np.array_equal(bits(made), bits(parsed))
    # ... and the parser's camera after set_resolution to that size
    s = sp.Scene.from_string(SCENE % (8, 8, text(eye), text(look), text(up), repr(fov)))
    s.set_resolution(w, h)
    assert np.array_equal(bits(made), bits(s.desc().camera))


def test_look_at_refusals():
    L = sp.lib()
    f3 = lambda *v: (C.c_float * 3)(*v)
    eye, look, up = f3(0, 0, 10), f3(0, 0, 0), f3(0, 1, 0)
    out = _abi.sp_camera_desc()
    call = lambda e=eye, l=look, u=up, fov=45.0, w=40, h=24, o=out: L.sp_camera_look_at(e, l, u, fov, w, h, None if o is None else C.byref(o))
    assert call() == 0
    for kw in ({"e": None}, {"l": None}, {"u": None}, {"o": None}):
        assert call(**kw) == ARG and b"null" in L.sp_last_error()
    for bad in (math.nan, math.inf, -math.inf):
        assert call(e=f3(0, bad, 10)) == ARG and b"finite" in L.sp_last_error()
        assert call(l=f3(bad, 0, 0)) == ARG
        assert call(u=f3(0, 1, bad)) == ARG
        assert call(fov=bad) == ARG
    for w, h in ((0, 24), (40, 0), (-1, 24), (65536, 24), (40, 65536)):
        assert call(w=w, h=h) == ARG and b"film size" in L.sp_last_error()
    assert call(w=1, h=65535) == 0
    for fov in (0.0, -1.0, 180.0, 200.0):
        assert call(fov=fov) == ARG and b"fov" in L.sp_last_error()
    assert call(fov=179.0) == 0
    with pytest.raises(sp.SimplePathError) as e:
        sp.camera_look_at((0, 0, 1), (0, 0, 0), (0, 1, 0), 0.0, 8, 8)
    assert e.value.code == ARG


def test_set_camera_on_a_scene_that_is_not_resident():
    L = sp.lib()
    eye, look, up, fov = CAMERAS[0]
    s = sp.Scene.from_string(SCENE % (40, 24, text(eye), text(look), text(up), repr(fov)))
    before = bits(s.desc().camera)
    other = sp.camera_look_at(*CAMERAS[1], 40, 24)
    # 1. null arguments; 2. the film size; 3. non-finite floats -- and nothing changes
    assert L.sp_scene_set_camera(None, C.byref(other)) == ARG and b"null" in L.sp_last_error()
    assert L.sp_scene_set_camera(s.handle, None) == ARG and b"null" in L.sp_last_error()
    wrong = sp.camera_look_at(*CAMERAS[1], 64, 40)
    wrong.transform.p[1] = math.nan  # the size is looked at first
    assert L.sp_scene_set_camera(s.handle, C.byref(wrong)) == ARG and b"film size" in L.sp_last_error()
    for field in ("vx", "vy", "vz", "p"):
        for bad in (math.nan, math.inf):
            c = sp.camera_look_at(*CAMERAS[1], 40, 24)
            getattr(c.transform, field)[2] = bad
            assert L.sp_scene_set_camera(s.handle, C.byref(c)) == ARG and b"finite" in L.sp_last_error()
    assert np.array_equal(bits(s.desc().camera), before)
    s.set_resolution(48, 32)  # the parsed camera does not fix the size
    s.set_resolution(40, 24)
    assert np.array_equal(bits(s.desc().camera), before)
    # the edit: the descriptor shows it, and the transform now fixes the image size
    s.set_camera(other)
    d = s.desc()
    assert np.array_equal(bits(d.camera), bits(other)) and (d.camera.film_width, d.camera.film_height) == (40, 24)
    with pytest.raises(sp.SimplePathError) as e:
        s.set_resolution(48, 32)
    assert e.value.code == STATE
    s.set_resolution(40, 24)  # the same size succeeds and keeps the camera
    assert np.array_equal(bits(s.desc().camera), bits(other))
    # a hand-made transform is taken as it is
    hand = _abi.sp_camera_desc()
    hand.transform.vx[:] = (1.0, 0.0, 0.0)
    hand.transform.vy[:] = (0.0, -1.0, 0.0)
    hand.transform.vz[:] = (-20.0, 12.0, -30.0)
    hand.transform.p[:] = (0.5, 0.25, 9.0)
    hand.film_width, hand.film_height = 40, 24
    s.set_camera(hand)
    assert np.array_equal(bits(s.desc().camera), bits(hand))
