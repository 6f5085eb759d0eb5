"""The refit surface of the C ABI without a device (include/simplepath_hip.h, SP_HAS_REFIT): the
header's announcement, struct layouts against the compiler's, and every refusal of
sp_scene_update_mesh / sp_scene_refit_build_check -- each returns its code and leaves the scene's
mesh as it was."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import simplepath_amd as sp
from simplepath_amd import _abi
from tests import _refit_moves as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "simplepath_hip.h")


def test_header_announces_the_surface():
    text = open(HEADER).read()
    assert re.search(r"^#define SP_HAS_REFIT 1\b", text, re.M)
    assert re.search(r"#define SP_ABI_VERSION 6\b", text)  # new entry points only
    for name in ("sp_scene_update_mesh", "sp_scene_refit_build_check"):
        assert name in _abi.SIGNATURES and hasattr(sp.lib(), name), name
    assert hasattr(sp.Scene, "update_mesh") and hasattr(sp.Scene, "refit_build_check")


def test_struct_layouts_match_the_compiler(tmp_path):
    U = ("struct_size", "reserved0", "vertices", "normals", "num_vertices", "reserved")
    S = ("struct_size", "refitted", "binary_passes", "wide_passes", "ms_copy", "ms_pack", "ms_binary", "ms_wide", "ms_total",
         "scratch_bytes")
    line = lambda t, fs: ('  printf("%zu' + " %zu" * len(fs) + '\\n", sizeof(' + t + ")"
                          + "".join(f", offsetof({t}, {f})" for f in fs) + ");\n")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "simplepath_hip.h"\nint main(void) {\n'
                   + line("sp_mesh_update", U) + line("sp_refit_stats", S) + "  return SP_HAS_REFIT - 1;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, timeout=120)
    a, b = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.splitlines()
    for got, T, fs in ((a, _abi.sp_mesh_update, U), (b, _abi.sp_refit_stats, S)):
        assert [int(x) for x in got.split()] == [C.sizeof(T)] + [getattr(T, f).offset for f in fs]
    assert C.sizeof(_abi.sp_mesh_update) == 48 and C.sizeof(_abi.sp_refit_stats) == 48


def update(v, **kw):
    u = _abi.sp_mesh_update()
    u.struct_size = C.sizeof(_abi.sp_mesh_update)
    u.vertices = v.ctypes.data_as(C.POINTER(C.c_float))
    u.num_vertices = v.shape[0]
    for k, val in kw.items():
        setattr(u, k, val)
    return u


def test_refusals_leave_the_mesh_unchanged(scene_dir):
    L = sp.lib()
    scene = sp.Scene.from_file(os.path.join(scene_dir, "bunny.sp"))
    before, f = R.mesh_of(scene)
    ptr = C.addressof(scene.desc().vertices.contents)
    moved = R.shift(before, f)
    short = np.ascontiguousarray(moved[:-1])
    null = C.POINTER(C.c_float)()
    st = _abi.sp_refit_stats()
    st.struct_size = C.sizeof(_abi.sp_refit_stats)
    bad_stats = _abi.sp_refit_stats()
    bad_stats.struct_size = 44
    bad = [update(moved, struct_size=0), update(moved, struct_size=C.sizeof(_abi.sp_mesh_update) + 8),
           update(moved, struct_size=C.sizeof(_abi.sp_mesh_update) - 4), update(moved, reserved0=1),
           update(moved, reserved=(C.c_int32 * 4)(0, 0, 0, 5)), update(moved, reserved=(C.c_int32 * 4)(1, 0, 0, 0)),
           update(moved, vertices=null), update(short), update(moved, num_vertices=moved.shape[0] + 1),
           update(moved, num_vertices=0), update(moved, num_vertices=-1)]
    for u in bad:
        assert L.sp_scene_update_mesh(scene.handle, C.byref(u), C.byref(st)) == _abi.SP_ERR_ARG
        assert L.sp_scene_update_mesh(scene.handle, C.byref(u), None) == _abi.SP_ERR_ARG
        assert L.sp_scene_refit_build_check(scene.handle, None, None, C.byref(u), None, None) == _abi.SP_ERR_ARG
        assert np.array_equal(R.mesh_of(scene)[0].view(np.uint32), before.view(np.uint32))
    good = update(moved)
    assert L.sp_scene_update_mesh(None, C.byref(good), None) == _abi.SP_ERR_ARG
    assert L.sp_scene_update_mesh(scene.handle, None, None) == _abi.SP_ERR_ARG
    assert L.sp_scene_update_mesh(scene.handle, C.byref(good), C.byref(bad_stats)) == _abi.SP_ERR_ARG
    assert L.sp_scene_refit_build_check(None, None, None, C.byref(good), None, None) == _abi.SP_ERR_ARG
    assert L.sp_scene_refit_build_check(scene.handle, None, None, None, None, None) == _abi.SP_ERR_ARG
    # the reference order is not refitted; a check struct of an unknown size is refused
    ref = _abi.sp_upload_params()
    ref.bvh_mode = 1
    assert L.sp_scene_refit_build_check(scene.handle, C.byref(ref), None, C.byref(good), None, None) == _abi.SP_ERR_ARG
    wrong = _abi.sp_bvh_check()
    wrong.struct_size = 8
    assert L.sp_scene_refit_build_check(scene.handle, None, None, C.byref(good), C.byref(wrong), None) == _abi.SP_ERR_ARG
    assert np.array_equal(R.mesh_of(scene)[0].view(np.uint32), before.view(np.uint32))
    # the check call does not modify the scene either; both out pointers may be NULL
    assert L.sp_scene_refit_build_check(scene.handle, None, None, C.byref(good), None, None) == _abi.SP_OK
    assert np.array_equal(R.mesh_of(scene)[0].view(np.uint32), before.view(np.uint32))
    # an accepted update of a scene that is not resident: the mesh in place, refitted 0
    assert L.sp_scene_update_mesh(scene.handle, C.byref(good), C.byref(st)) == _abi.SP_OK
    assert st.refitted == 0 and st.binary_passes == 0 and st.scratch_bytes == 0
    assert C.addressof(scene.desc().vertices.contents) == ptr  # pointers from an earlier desc() stay valid
    assert np.array_equal(R.mesh_of(scene)[0].view(np.uint32), moved.view(np.uint32))


def test_normals_are_optional(scene_dir):
    scene = sp.Scene.from_file(os.path.join(scene_dir, "bunny.sp"))
    d = scene.desc()
    nv = d.info.num_vertices
    n0 = np.ctypeslib.as_array(d.normals, shape=(nv, 3)).copy()
    v, f = R.mesh_of(scene)
    assert scene.update_mesh(R.shift(v, f)) is None
    assert np.array_equal(np.ctypeslib.as_array(scene.desc().normals, shape=(nv, 3)), n0)
    st = scene.update_mesh(v, normals=-n0, stats=True)
    assert st["refitted"] == 0
    assert np.array_equal(np.ctypeslib.as_array(scene.desc().normals, shape=(nv, 3)), -n0)
    assert np.array_equal(R.mesh_of(scene)[0], v)


def test_a_scene_without_vertices_is_a_no_op(tmp_path):
    from tests import _lbvh_sets
    scene = sp.Scene.from_file(_lbvh_sets.write_set(str(tmp_path), "balls", None, [(0.0, 0.0, 0.0, 0.3), (0.5, 0.2, 0.1, 0.1)]))
    assert scene.info().num_vertices == 0
    assert scene.update_mesh(np.zeros((0, 3), np.float32), stats=True)["refitted"] == 0
    u = _abi.sp_mesh_update()
    u.struct_size = C.sizeof(_abi.sp_mesh_update)
    assert sp.lib().sp_scene_update_mesh(scene.handle, C.byref(u), None) == _abi.SP_OK
    u.num_vertices = 1
    assert sp.lib().sp_scene_update_mesh(scene.handle, C.byref(u), None) == _abi.SP_ERR_ARG
    b, w = scene.refit_build_check(np.zeros((0, 3), np.float32))
    assert b["errors"] == 0 and w["errors"] == 0 and b["slots"] == 2
