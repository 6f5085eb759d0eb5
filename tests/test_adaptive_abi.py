"""The adaptive-sampling surface of the C ABI (include/simplepath_hip.h, SP_HAS_ADAPTIVE): the header's
announcement, struct layouts against the compiler's on the header, the errors that come back before
any device is touched, and (on a GPU) tests/cpp/adaptive_main.cpp -- sp_amd::render_adaptive compiled
and linked as a host program would -- against the Python binding."""
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
LIBDIR = os.path.join(ROOT, "simplepath_amd", "_build")
NAMES = ("sp_progress_create_adaptive", "sp_adaptive_round", "sp_adaptive_round_host", "sp_adaptive_tile_samples",
         "sp_adaptive_tile_errors", "sp_adaptive_export", "sp_adaptive_import")


def test_header_announces_the_surface():
    text = open(HEADER).read()
    assert re.search(r"^#define SP_HAS_ADAPTIVE 1\b", text, re.M)
    assert re.search(r"^#define SP_HAS_PROGRESS 1\b", text, re.M)
    assert re.search(r"#define SP_ABI_VERSION 6\b", text)  # new entry points only
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in _abi.SIGNATURES and hasattr(sp.lib(), name), name


def test_struct_layouts_match_the_compiler(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "simplepath_hip.h"\n'
        "int main(void) {\n"
        '  printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(sp_adaptive_params), offsetof(sp_adaptive_params, threshold),\n'
        "         offsetof(sp_adaptive_params, min_samples), offsetof(sp_adaptive_params, max_samples),\n"
        "         offsetof(sp_adaptive_params, step), offsetof(sp_adaptive_params, floor), offsetof(sp_adaptive_params, reserved));\n"
        '  printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(sp_adaptive_result), offsetof(sp_adaptive_result, samples_total),\n'
        "         offsetof(sp_adaptive_result, min_done), offsetof(sp_adaptive_result, max_done),\n"
        "         offsetof(sp_adaptive_result, max_error), offsetof(sp_adaptive_result, reserved));\n"
        '  printf("%zu %zu %zu\\n", sizeof(sp_pixel_noise), offsetof(sp_pixel_noise, m2), sizeof(sp_progress_params));\n'
        "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, timeout=120)
    a, b, c = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.splitlines()
    P, R, N = _abi.sp_adaptive_params, _abi.sp_adaptive_result, _abi.sp_pixel_noise
    assert [int(x) for x in a.split()] == [C.sizeof(P), P.threshold.offset, P.min_samples.offset, P.max_samples.offset,
                                           P.step.offset, P.floor.offset, P.reserved.offset] == [32, 4, 8, 12, 16, 20, 24]
    assert [int(x) for x in b.split()] == [C.sizeof(R), R.samples_total.offset, R.min_done.offset, R.max_done.offset,
                                           R.max_error.offset, R.reserved.offset] == [32, 8, 16, 20, 24, 28]
    assert [int(x) for x in c.split()] == [C.sizeof(N), N.m2.offset, C.sizeof(_abi.sp_progress_params)] == [8, 4, 48]
    d = sp.PIXEL_NOISE_DTYPE
    assert d.itemsize == 8 and [d.fields[k][1] for k in ("mean", "m2")] == [0, 4]


def test_errors_without_a_device(scene_dir):
    L = sp.lib()
    scene = sp.Scene.from_file(os.path.join(scene_dir, "bunny.sp"))
    h = C.c_void_p()
    p = _abi.sp_progress_params()
    p.struct_size = C.sizeof(p)
    # a scene that is not uploaded; null arguments; the parameter checks of sp_progress_create
    assert L.sp_progress_create_adaptive(scene.handle, C.byref(p), C.byref(h)) == _abi.SP_ERR_STATE
    assert not h.value
    assert L.sp_progress_create_adaptive(None, C.byref(p), C.byref(h)) == _abi.SP_ERR_ARG
    assert L.sp_progress_create_adaptive(scene.handle, None, C.byref(h)) == _abi.SP_ERR_ARG
    assert L.sp_progress_create_adaptive(scene.handle, C.byref(p), None) == _abi.SP_ERR_ARG
    p.struct_size = 0
    assert L.sp_progress_create_adaptive(scene.handle, C.byref(p), C.byref(h)) == _abi.SP_ERR_ARG
    a = sp.Progressive._adaptive_params(0.1, 1, 4, 1, 0.0)
    assert a.struct_size == 32
    buf = (C.c_uint32 * 4)()
    fbuf = (C.c_float * 4)()
    assert L.sp_adaptive_round(None, C.byref(a), None, None, None, None) == _abi.SP_ERR_ARG
    assert L.sp_adaptive_round_host(None, C.byref(a), fbuf, None, None) == _abi.SP_ERR_ARG
    assert L.sp_adaptive_tile_samples(None, buf, 4) == _abi.SP_ERR_ARG
    assert L.sp_adaptive_tile_errors(None, 0.0, fbuf, 4) == _abi.SP_ERR_ARG
    assert L.sp_adaptive_export(None, None, 0, buf, 4) == _abi.SP_ERR_ARG
    assert L.sp_adaptive_import(None, None, 0, buf, 4) == _abi.SP_ERR_ARG
    assert b"null" in L.sp_last_error()


def read_pfm(path):
    with open(path, "rb") as fh:
        assert fh.readline().strip() == b"PF"
        w, h = (int(x) for x in fh.readline().split())
        scale = float(fh.readline())
        data = np.frombuffer(fh.read(), dtype="<f4" if scale < 0 else ">f4")
    return data.reshape(h, w, 3)[::-1]  # rows bottom-up in the file (Image/Image.cpp:40)


@pytest.mark.gpu
def test_render_adaptive_drop_in_matches_python(scene_dir, tmp_path):
    exe = str(tmp_path / "adaptive_main")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "adaptive_main.cpp"), "-o", exe,
                    "-L", LIBDIR, "-lsimplepath_hip", f"-Wl,-rpath,{LIBDIR}"], check=True, timeout=600)
    out, cnt = str(tmp_path / "img.pfm"), str(tmp_path / "counts.u32")
    path = os.path.join(scene_dir, "bunny.sp")
    r = subprocess.run([exe, path, "--rule", "0.05", "2", "11", "3", "--integrator", "direct_lighting", "--bvh", "1",
                        "--size", "40", "60", "--output", out, "--counts", cnt], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    s = sp.Scene.from_file(path)
    s.set_resolution(40, 60)
    s.upload(device=0, bvh_mode=1)
    with sp.Progressive(s, "direct_lighting", adaptive=True) as prog:
        tiles, rounds = prog.converge(0.05, 2, 11, 3)
        done = prog.tile_samples()
    assert len(set(done.tolist())) > 1
    assert np.array_equal(np.fromfile(cnt, dtype=np.uint32), done)
    ref = sp.tiles_to_image(40, 60, tiles)
    assert np.array_equal(read_pfm(out).view(np.uint32), ref.view(np.uint32))
    assert f"{len(rounds)} rounds, {rounds[-1][1].samples_total} samples" in r.stdout
