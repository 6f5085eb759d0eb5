"""The progressive-render surface of the C ABI without a device (include/simplepath_hip.h,
SP_HAS_PROGRESS): struct layouts against the compiler's on the header, argument and state errors
that come back before any device is touched, and the checkpoint format's claim -- sp_pixel_state's
mt / mt_pos are std::mt19937_64's own words and position -- checked by tests/cpp/mt_continue_check.cpp
on states it takes from std::mt19937_64 itself."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import simplepath_amd as sp
from simplepath_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "simplepath_hip.h")


def params(**kw):
    p = _abi.sp_progress_params()
    p.struct_size = C.sizeof(_abi.sp_progress_params)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_header_announces_the_surface():
    text = open(HEADER).read()
    assert re.search(r"^#define SP_HAS_PROGRESS 1\b", text, re.M)
    assert re.search(r"#define SP_ABI_VERSION 6\b", text)  # new entry points only
    for name in ("sp_progress_create", "sp_progress_free", "sp_progress_render", "sp_progress_samples",
                 "sp_progress_device_bytes", "sp_progress_export", "sp_progress_import"):
        assert name in _abi.SIGNATURES and hasattr(sp.lib(), name), name


def test_struct_layouts_match_the_compiler(tmp_path):
    assert C.sizeof(_abi.sp_pixel_state) == 2528
    assert sp.PIXEL_STATE_DTYPE.itemsize == 2528
    src = tmp_path / "layout.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "simplepath_hip.h"\n'
        "int main(void) {\n"
        '  printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(sp_progress_params), offsetof(sp_progress_params, integrator),\n'
        "         offsetof(sp_progress_params, tile_ids), offsetof(sp_progress_params, d_tile_ids),\n"
        "         offsetof(sp_progress_params, num_tiles), offsetof(sp_progress_params, waves_per_simd),\n"
        "         offsetof(sp_progress_params, tile_order_factor), offsetof(sp_progress_params, reserved));\n"
        '  printf("%zu %zu %zu %zu %zu\\n", sizeof(sp_pixel_state), offsetof(sp_pixel_state, mt_pos),\n'
        "         offsetof(sp_pixel_state, draws), offsetof(sp_pixel_state, sum), offsetof(sp_pixel_state, reserved));\n"
        "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, timeout=120)
    a, b = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.splitlines()
    P, S = _abi.sp_progress_params, _abi.sp_pixel_state
    assert [int(x) for x in a.split()] == [C.sizeof(P), P.integrator.offset, P.tile_ids.offset, P.d_tile_ids.offset,
                                           P.num_tiles.offset, P.waves_per_simd.offset, P.tile_order_factor.offset,
                                           P.reserved.offset]
    assert [int(x) for x in b.split()] == [C.sizeof(S), S.mt_pos.offset, S.draws.offset, S.sum.offset, S.reserved.offset]
    d = sp.PIXEL_STATE_DTYPE
    assert [d.fields[k][1] for k in ("mt", "mt_pos", "draws", "sum", "reserved")] == \
        [S.mt.offset, S.mt_pos.offset, S.draws.offset, S.sum.offset, S.reserved.offset]


def test_create_argument_and_state_errors(scene_dir):
    L = sp.lib()
    scene = sp.Scene.from_file(os.path.join(scene_dir, "bunny.sp"))
    h = C.c_void_p()
    good = params()
    # a scene that is not uploaded
    assert L.sp_progress_create(scene.handle, C.byref(good), C.byref(h)) == _abi.SP_ERR_STATE
    assert not h.value
    # NULL arguments
    assert L.sp_progress_create(None, C.byref(good), C.byref(h)) == _abi.SP_ERR_ARG
    assert L.sp_progress_create(scene.handle, None, C.byref(h)) == _abi.SP_ERR_ARG
    assert L.sp_progress_create(scene.handle, C.byref(good), None) == _abi.SP_ERR_ARG
    # a struct_size the library does not know, reserved words, both lists, NaN
    for bad in (params(struct_size=0), params(struct_size=C.sizeof(_abi.sp_progress_params) + 8),
                params(struct_size=C.sizeof(_abi.sp_progress_params) - 4),
                params(reserved=(C.c_int32 * 2)(1, 0)), params(reserved=(C.c_int32 * 2)(0, 7)),
                params(tile_order_factor=float("nan"))):
        assert L.sp_progress_create(scene.handle, C.byref(bad), C.byref(h)) == _abi.SP_ERR_ARG
        assert not h.value
    ids = np.arange(3, dtype=np.int32)
    both = params(tile_ids=ids.ctypes.data_as(C.POINTER(C.c_int32)), d_tile_ids=64, num_tiles=3)
    assert L.sp_progress_create(scene.handle, C.byref(both), C.byref(h)) == _abi.SP_ERR_ARG
    # the other entry points on a NULL handle
    n, b = C.c_uint32(), C.c_int64()
    assert L.sp_progress_render(None, 1, None, None, None) == _abi.SP_ERR_ARG
    assert L.sp_progress_samples(None, C.byref(n)) == _abi.SP_ERR_ARG
    assert L.sp_progress_device_bytes(None, C.byref(b)) == _abi.SP_ERR_ARG
    assert L.sp_progress_export(None, None, 0, C.byref(n)) == _abi.SP_ERR_ARG
    assert L.sp_progress_import(None, None, 0, 0) == _abi.SP_ERR_ARG
    L.sp_progress_free(None)  # like free()
    # the Python wrapper raises the same state error
    try:
        sp.Progressive(scene, "direct_lighting")
        raise AssertionError("expected SP_ERR_STATE")
    except sp.SimplePathError as e:
        assert e.code == _abi.SP_ERR_STATE


def test_mt_continue_check_self(tmp_path):
    # plain g++ -std=c++17; on states std::mt19937_64 printed itself it must report 0 mismatches
    # (and it refuses a corrupted one)
    exe = str(tmp_path / "mt_continue_check")
    subprocess.run(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "cpp", "mt_continue_check.cpp"), "-o", exe],
                   check=True, timeout=300)
    r = subprocess.run([exe, "--self"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"^24 records, 0 mismatching$", r.stdout, re.M), r.stdout
