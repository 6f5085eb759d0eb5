"""The feature-buffer surface without a device (include/simplepath_hip.h, "feature buffers"): the
structs' layouts in C and ctypes, the announcement in the header, and every refusal of
sp_scene_camera_rays and sp_scene_features in the order the header states, on a scene that is not
resident -- so the residency check, which comes last, answers only once everything else is in order."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import simplepath_amd as sp
from simplepath_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "simplepath_hip.h")
NAMES = ("sp_scene_camera_rays", "sp_scene_camera_rays_host", "sp_scene_features", "sp_scene_features_host")
ARG, STATE = _abi.SP_ERR_ARG, _abi.SP_ERR_STATE
ALIGNED, ODD = 0x1000, 0x1008  # stand-in device addresses: validation never reads through them
OUTPUTS = ("d_ids", "d_coverage", "d_depth", "d_normal", "d_albedo")


def test_header_announces_the_surface():
    text = open(HEADER).read()
    assert re.search(r"^#define SP_HAS_FEATURES 1\b", text, re.M)
    assert re.search(r"#define SP_ABI_VERSION 6\b", text)  # new entry points only
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in _abi.SIGNATURES and hasattr(sp.lib(), name), name
    for name in ("FEATURE_IDS_DTYPE", "FEATURE_OUTPUTS"):
        assert name in sp.__all__
    assert sp.FEATURE_IDS_DTYPE.itemsize == 16 and sp.FEATURE_IDS_DTYPE.names == ("kind", "index", "material", "hits")
    assert "lights are not intersected" in text  # the header states that the buffers are geometry only


def fields(struct):
    return [C.sizeof(struct)] + [getattr(struct, name).offset for name, _ in struct._fields_[1:]]


def test_struct_layouts_match_the_compiler(tmp_path):
    structs = (_abi.sp_camera_ray_params, _abi.sp_feature_params, _abi.sp_feature_stats)
    lines = []
    for s in structs:
        name = s.__name__
        offs = ", ".join(f"offsetof({name}, {f})" for f, _ in s._fields_[1:])
        lines.append(f'  printf("%zu{" %zu" * (len(s._fields_) - 1)}\\n", sizeof({name}), {offs});\n')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "simplepath_hip.h"\nint main(void) {\n' + "".join(lines)
                   + "  return SP_HAS_FEATURES == 1 ? 0 : 1;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, timeout=120)
    out = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.splitlines()
    for s, line in zip(structs, out):
        assert [int(x) for x in line.split()] == fields(s), s.__name__
    assert [C.sizeof(s) for s in structs] == [72, 120, 32]  # the sizes the header states


def ray_params(n_tiles=0, samples=2, first=0):
    p = _abi.sp_camera_ray_params()
    p.struct_size = C.sizeof(p)
    p.first_sample, p.num_samples, p.num_tiles = first, samples, n_tiles
    return p


def feature_params(n_tiles=0, samples=2, **pointers):
    p = _abi.sp_feature_params()
    p.struct_size = C.sizeof(p)
    p.samples_per_pixel, p.num_tiles = samples, n_tiles
    for name, value in (pointers or {"d_depth": ALIGNED}).items():
        setattr(p, name, value or None)
    return p


@pytest.fixture(scope="module")
def scene(scene_dir):
    s = sp.Scene.from_file(os.path.join(scene_dir, "bunny.sp"))  # never uploaded
    s.set_resolution(20, 12)  # 3 x 2 tiles
    return s


def stats(size=None):
    st = _abi.sp_feature_stats()
    st.struct_size = C.sizeof(st) if size is None else size
    return st


def shared_refusals(scene, call, make, what):
    """the refusals both calls share, in order; make(): parameters that only lack the residency"""
    L = sp.lib()
    ids = (C.c_int32 * 3)(0, 5, 2)
    bad_ids = (C.c_int32 * 3)(0, 6, 2)
    assert call(scene.handle, make()) == STATE and b"sp_scene_upload" in L.sp_last_error(), what
    # 1. null scene or params -- before anything in them is looked at
    p = make()
    p.struct_size = 0
    assert call(None, p) == ARG and b"null" in L.sp_last_error()
    assert call(scene.handle, None) == ARG and b"null" in L.sp_last_error()
    # 2. struct sizes and reserved words -- before the counts
    p = make()
    p.struct_size, p.num_tiles = C.sizeof(p) - 8, -1
    assert call(scene.handle, p) == ARG and b"struct_size" in L.sp_last_error()
    assert call(scene.handle, make(), stats(0)) == ARG and b"sp_feature_stats" in L.sp_last_error()
    assert call(scene.handle, make(), stats()) == STATE
    for k in range(4):
        p = make()
        p.reserved[k], p.num_tiles = 1, -1
        assert call(scene.handle, p) == ARG and b"reserved" in L.sp_last_error()
    # 3. negative counts, then the tile-list rules -- before the pointers
    p = make()
    p.tile_ids, p.num_tiles = ids, -1
    assert call(scene.handle, p) == ARG and b"num_tiles" in L.sp_last_error()
    p = make()
    p.tile_ids, p.d_tile_ids, p.num_tiles = ids, ALIGNED, 3
    assert call(scene.handle, p) == ARG and b"not both" in L.sp_last_error()
    p = make()
    p.tile_ids, p.num_tiles = bad_ids, 3
    assert call(scene.handle, p) == ARG and b"out of range" in L.sp_last_error()
    p = make()
    p.tile_ids, p.num_tiles = ids, 3
    assert call(scene.handle, p) == STATE
    p = make()
    p.d_tile_ids, p.num_tiles = ALIGNED, 3
    assert call(scene.handle, p) == STATE
    # the camera override: the scene's film size, finite floats
    cam = sp.camera_look_at((0, 0, 3), (0, 0, 0), (0, 1, 0), 40.0, 24, 12)
    p = make()
    p.camera = C.pointer(cam)
    assert call(scene.handle, p) == ARG and b"film size" in L.sp_last_error()
    cam = sp.camera_look_at((0, 0, 3), (0, 0, 0), (0, 1, 0), 40.0, 20, 12)
    p.camera = C.pointer(cam)
    assert call(scene.handle, p) == STATE
    cam.transform.vy[1] = float("nan")
    assert call(scene.handle, p) == ARG and b"finite" in L.sp_last_error()


def test_camera_rays_refuse_in_the_stated_order(scene):
    L = sp.lib()

    def call(s, p, st=None, rays=ALIGNED):
        return L.sp_scene_camera_rays(s, None if p is None else C.byref(p), rays or None, None if st is None else C.byref(st))
    shared_refusals(scene, call, ray_params, "camera rays")
    reserved0 = ray_params()
    reserved0.reserved0 = 1
    assert call(scene.handle, reserved0) == ARG and b"reserved" in L.sp_last_error()
    assert call(scene.handle, ray_params(first=0xffffffff, samples=2)) == ARG and b"2^32" in L.sp_last_error()
    assert call(scene.handle, ray_params(first=0xffffffff, samples=1)) == STATE
    # no output pointer, then a misaligned one -- before the residency
    assert call(scene.handle, ray_params(), rays=0) == ARG and b"output" in L.sp_last_error()
    assert call(scene.handle, ray_params(samples=0), rays=0) == STATE  # nothing to write: "succeeds" comes after the residency
    assert call(scene.handle, ray_params(), rays=ODD) == ARG and b"aligned" in L.sp_last_error()
    # the host form refuses alike, and asks no alignment of a host array
    host = np.zeros((6, 2, 64), dtype=sp.RAY_DTYPE)
    hcall = lambda s, p, r: L.sp_scene_camera_rays_host(s, None if p is None else C.byref(p), r, None)
    assert hcall(None, ray_params(), C.c_void_p(host.ctypes.data)) == ARG
    assert hcall(scene.handle, None, C.c_void_p(host.ctypes.data)) == ARG
    assert hcall(scene.handle, ray_params(), None) == ARG
    assert hcall(scene.handle, ray_params(n_tiles=-1), C.c_void_p(host.ctypes.data)) == ARG  # refused even without a list
    assert hcall(scene.handle, ray_params(), C.c_void_p(host.ctypes.data + 4)) == STATE
    with pytest.raises(sp.SimplePathError) as e:
        scene.camera_rays()
    assert e.value.code == STATE
    with pytest.raises(sp.SimplePathError) as e:
        scene.camera_rays_device(ODD)
    assert e.value.code == ARG


def test_features_refuse_in_the_stated_order(scene):
    L = sp.lib()
    call = lambda s, p, st=None: L.sp_scene_features(s, None if p is None else C.byref(p), None if st is None else C.byref(st))
    shared_refusals(scene, call, feature_params, "features")
    counts = (C.c_uint32 * 6)(1, 2, 3, 4, 5, 6)
    p = feature_params()
    p.tile_samples, p.d_tile_samples = counts, ALIGNED
    assert call(scene.handle, p) == ARG and b"not both" in L.sp_last_error()
    p.d_tile_samples = None
    assert call(scene.handle, p) == STATE
    # no output pointer -- before the alignment
    none = feature_params(d_depth=0)
    none.d_tile_samples = ALIGNED + 2
    assert call(scene.handle, none) == ARG and b"output" in L.sp_last_error()
    # each single output is enough; d_ids needs 16 bytes, the others 4
    for name in OUTPUTS:
        assert call(scene.handle, feature_params(**{name: ALIGNED})) == STATE, name
        assert call(scene.handle, feature_params(**{name: ALIGNED + 2})) == ARG and b"aligned" in L.sp_last_error(), name
        assert call(scene.handle, feature_params(**{name: ALIGNED + 4})) == (ARG if name == "d_ids" else STATE), name
    assert call(scene.handle, feature_params(d_ids=ODD, d_depth=ALIGNED)) == ARG and b"d_ids" in L.sp_last_error()
    assert call(scene.handle, feature_params(**{name: ALIGNED for name in OUTPUTS})) == STATE
    assert call(scene.handle, feature_params(samples=0)) == STATE  # n == 0 is a count like any other
    # the host form refuses alike, and asks no alignment of host arrays
    hcall = lambda s, p: L.sp_scene_features_host(s, None if p is None else C.byref(p), None)
    depth = np.zeros((6, 64), dtype=np.float32)
    assert hcall(None, feature_params(d_depth=depth.ctypes.data)) == ARG
    assert hcall(scene.handle, None) == ARG
    assert hcall(scene.handle, feature_params(d_depth=0)) == ARG
    assert hcall(scene.handle, feature_params(d_ids=depth.ctypes.data + 4)) == STATE
    with pytest.raises(sp.SimplePathError) as e:
        scene.features(2)
    assert e.value.code == STATE
    with pytest.raises(sp.SimplePathError) as e:
        scene.features_device(2)  # no output pointer
    assert e.value.code == ARG
    with pytest.raises(ValueError):
        scene.features(2, outputs=("depth", "colour"))
    with pytest.raises(ValueError):
        scene.features(2, tile_samples=[1, 2, 3])  # six slots
