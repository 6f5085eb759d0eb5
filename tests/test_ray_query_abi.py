"""The ray-query surface without a device (include/simplepath_hip.h, "ray queries"): the records'
layouts in C, ctypes and numpy, the announcement in the header, and every refusal of
sp_scene_trace_rays in the order the header states, on a scene that is not resident -- so the
residency check, which comes last, answers only once everything else is in order."""
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
NAMES = ("sp_scene_trace_rays", "sp_scene_trace_rays_host")
ARG, STATE = _abi.SP_ERR_ARG, _abi.SP_ERR_STATE
ALIGNED, ODD = 0x1000, 0x1008  # stand-in device addresses: validation never reads through them


def test_header_announces_the_surface():
    text = open(HEADER).read()
    assert re.search(r"^#define SP_HAS_RAY_QUERY 1\b", text, re.M)
    assert re.search(r"#define SP_ABI_VERSION 6\b", text)  # new entry points only
    assert re.search(r"enum \{ SP_QUERY_CLOSEST = 0, SP_QUERY_ANY = 1 \}", text)
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in _abi.SIGNATURES and hasattr(sp.lib(), name), name
    for name in ("RAY_DTYPE", "RAY_HIT_DTYPE"):
        assert name in sp.__all__


def test_records_are_32_bytes_in_ctypes_and_numpy():
    assert C.sizeof(_abi.sp_ray) == 32 and C.sizeof(_abi.sp_ray_hit) == 32
    for dtype, struct in ((sp.RAY_DTYPE, _abi.sp_ray), (sp.RAY_HIT_DTYPE, _abi.sp_ray_hit)):
        assert dtype.itemsize == C.sizeof(struct) == 32
        assert list(dtype.names) == [name for name, _ in struct._fields_]
        for name, ctype in struct._fields_:
            field = getattr(struct, name)
            sub, offset = dtype.fields[name][:2]
            assert offset == field.offset and sub.itemsize == field.size, name
            scalar = ctype._type_ if hasattr(ctype, "_length_") else ctype
            assert sub.base == np.dtype(scalar), name


def test_struct_layouts_match_the_compiler(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "simplepath_hip.h"\n'
        "int main(void) {\n"
        '  printf("%zu %zu %zu %zu\\n", sizeof(sp_ray), offsetof(sp_ray, tmin), offsetof(sp_ray, d), offsetof(sp_ray, tmax));\n'
        '  printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(sp_ray_hit), offsetof(sp_ray_hit, kind), offsetof(sp_ray_hit, index),\n'
        "         offsetof(sp_ray_hit, material), offsetof(sp_ray_hit, beta), offsetof(sp_ray_hit, gamma),\n"
        "         offsetof(sp_ray_hit, reserved));\n"
        '  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(sp_ray_query), offsetof(sp_ray_query, mode),\n'
        "         offsetof(sp_ray_query, d_rays), offsetof(sp_ray_query, num_rays), offsetof(sp_ray_query, stream),\n"
        "         offsetof(sp_ray_query, d_hits), offsetof(sp_ray_query, d_normals), offsetof(sp_ray_query, d_occluded),\n"
        "         offsetof(sp_ray_query, reserved));\n"
        '  printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(sp_ray_query_stats), offsetof(sp_ray_query_stats, launches),\n'
        "         offsetof(sp_ray_query_stats, rays), offsetof(sp_ray_query_stats, hits),\n"
        "         offsetof(sp_ray_query_stats, kernel_ms), offsetof(sp_ray_query_stats, stack_depth));\n"
        "  return SP_HAS_RAY_QUERY == 1 && SP_QUERY_CLOSEST == 0 && SP_QUERY_ANY == 1 ? 0 : 1;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, timeout=120)
    a, b, c, d = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.splitlines()
    R, H, Q, S = _abi.sp_ray, _abi.sp_ray_hit, _abi.sp_ray_query, _abi.sp_ray_query_stats
    assert [int(x) for x in a.split()] == [C.sizeof(R), R.tmin.offset, R.d.offset, R.tmax.offset] == [32, 12, 16, 28]
    assert [int(x) for x in b.split()] == [C.sizeof(H), H.kind.offset, H.index.offset, H.material.offset, H.beta.offset,
                                           H.gamma.offset, H.reserved.offset] == [32, 4, 8, 12, 16, 20, 24]
    assert [int(x) for x in c.split()] == [C.sizeof(Q), Q.mode.offset, Q.d_rays.offset, Q.num_rays.offset, Q.stream.offset,
                                           Q.d_hits.offset, Q.d_normals.offset, Q.d_occluded.offset,
                                           Q.reserved.offset] == [72, 4, 8, 16, 24, 32, 40, 48, 56]
    assert [int(x) for x in d.split()] == [C.sizeof(S), S.launches.offset, S.rays.offset, S.hits.offset, S.kernel_ms.offset,
                                           S.stack_depth.offset] == [32, 4, 8, 16, 24, 28]


def query(mode=_abi.SP_QUERY_CLOSEST, n=4, rays=ALIGNED, hits=0, normals=0, occluded=0):
    q = _abi.sp_ray_query()
    q.struct_size = C.sizeof(q)
    q.mode, q.num_rays = mode, n
    q.d_rays, q.d_hits, q.d_normals, q.d_occluded = rays or None, hits or None, normals or None, occluded or None
    return q


@pytest.fixture(scope="module")
def scene(scene_dir):
    return sp.Scene.from_file(os.path.join(scene_dir, "bunny.sp"))  # never uploaded


def test_refusals_come_in_the_stated_order(scene):
    L = sp.lib()
    call = lambda s, q, st=None: L.sp_scene_trace_rays(s, None if q is None else C.byref(q), None if st is None else C.byref(st))
    closest = lambda **kw: query(_abi.SP_QUERY_CLOSEST, hits=ALIGNED, **kw)
    anyhit = lambda **kw: query(_abi.SP_QUERY_ANY, occluded=ALIGNED, **kw)
    # everything in order: only the residency is missing, for both modes, with and without normals
    assert call(scene.handle, closest()) == STATE
    assert b"sp_scene_upload" in L.sp_last_error()
    assert call(scene.handle, closest(normals=ALIGNED)) == STATE
    assert call(scene.handle, anyhit()) == STATE
    assert call(scene.handle, anyhit(n=0)) == STATE  # "num_rays == 0 succeeds" comes after the residency
    # 1. null scene or query -- before anything in the query is looked at
    bad = closest()
    bad.struct_size = 0
    assert call(None, bad) == ARG and b"null" in L.sp_last_error()
    assert call(scene.handle, None) == ARG and b"null" in L.sp_last_error()
    # 2. struct_size and reserved words -- before the mode
    q = closest()
    q.struct_size, q.mode = C.sizeof(q) - 8, 7
    assert call(scene.handle, q) == ARG and b"struct_size" in L.sp_last_error()
    for k in range(4):
        q = closest()
        q.reserved[k], q.mode = 1, 7
        assert call(scene.handle, q) == ARG and b"reserved" in L.sp_last_error()
    st = _abi.sp_ray_query_stats()  # struct_size left 0
    assert call(scene.handle, closest(), st) == ARG and b"sp_ray_query_stats" in L.sp_last_error()
    st.struct_size = C.sizeof(st)
    assert call(scene.handle, closest(), st) == STATE
    # 3. unknown mode -- before the count
    for mode in (-1, 2, 7):
        q = query(mode, n=-1)
        assert call(scene.handle, q) == ARG and b"mode" in L.sp_last_error()
    # 4. num_rays < 0 -- before the pointers
    assert call(scene.handle, query(_abi.SP_QUERY_CLOSEST, n=-1)) == ARG and b"num_rays" in L.sp_last_error()
    assert call(scene.handle, query(_abi.SP_QUERY_ANY, n=-1, hits=ALIGNED)) == ARG and b"num_rays" in L.sp_last_error()
    # 5. the pointer rules of each mode: missing, forbidden, misaligned -- before the residency
    assert call(scene.handle, closest(rays=0)) == ARG                                  # no rays
    assert call(scene.handle, query(_abi.SP_QUERY_CLOSEST)) == ARG                     # no hits
    assert call(scene.handle, closest(occluded=ALIGNED)) == ARG                        # forbidden
    assert call(scene.handle, query(_abi.SP_QUERY_ANY)) == ARG                         # no occlusion words
    assert call(scene.handle, anyhit(hits=ALIGNED)) == ARG                             # forbidden
    assert call(scene.handle, anyhit(normals=ALIGNED)) == ARG                          # forbidden
    assert call(scene.handle, anyhit(n=0, hits=ALIGNED)) == ARG                        # forbidden at any count
    assert call(scene.handle, closest(rays=ODD)) == ARG and b"aligned" in L.sp_last_error()
    assert call(scene.handle, query(_abi.SP_QUERY_CLOSEST, hits=ODD)) == ARG and b"aligned" in L.sp_last_error()
    assert call(scene.handle, closest(normals=ODD)) == ARG and b"aligned" in L.sp_last_error()
    assert call(scene.handle, anyhit(rays=ODD)) == ARG and b"aligned" in L.sp_last_error()
    assert call(scene.handle, query(_abi.SP_QUERY_ANY, occluded=ALIGNED + 4)) == STATE # a word needs no 16 bytes
    assert call(scene.handle, query(_abi.SP_QUERY_ANY, occluded=ALIGNED + 2)) == ARG and b"aligned" in L.sp_last_error()
    # 6. SP_ERR_STATE is last: nothing above was wrong with these


def test_the_host_variant_refuses_alike(scene):
    L = sp.lib()
    rays = np.zeros(4, dtype=sp.RAY_DTYPE)
    hits = np.zeros(4, dtype=sp.RAY_HIT_DTYPE)
    occ = np.zeros(4, dtype=np.uint32)
    host = lambda s, mode, r, n, h, nr, o: L.sp_scene_trace_rays_host(s, mode, r, n, h, nr, o, None)
    p = lambda a: C.c_void_p(a.ctypes.data)
    assert host(None, 0, p(rays), 4, p(hits), None, None) == ARG
    assert host(scene.handle, 5, p(rays), 4, p(hits), None, None) == ARG
    assert host(scene.handle, 0, p(rays), -1, p(hits), None, None) == ARG
    assert host(scene.handle, 0, None, 4, p(hits), None, None) == ARG
    assert host(scene.handle, 0, p(rays), 4, None, None, None) == ARG
    assert host(scene.handle, 0, p(rays), 4, p(hits), None, p(occ)) == ARG
    assert host(scene.handle, 1, p(rays), 4, p(hits), None, p(occ)) == ARG
    assert host(scene.handle, 1, p(rays), 4, None, None, None) == ARG
    assert host(scene.handle, 0, p(rays), 4, p(hits), None, None) == STATE
    assert host(scene.handle, 1, p(rays), 4, None, None, p(occ)) == STATE
    # the Python wrappers raise the same codes
    with pytest.raises(sp.SimplePathError) as e:
        scene.trace(np.zeros((3, 3)), np.ones((3, 3)))
    assert e.value.code == STATE
    with pytest.raises(sp.SimplePathError) as e:
        scene.trace_device(ALIGNED, 3, hits_ptr=ALIGNED, occluded_ptr=ALIGNED)
    assert e.value.code == ARG


def test_make_rays_broadcasts_the_limits():
    o = np.arange(15, dtype=np.float64).reshape(5, 3)
    r = sp.make_rays(o, -o, tmax=np.arange(5))
    assert r.dtype == sp.RAY_DTYPE and r.shape == (5,)
    assert np.array_equal(r["o"], o.astype(np.float32)) and np.array_equal(r["d"], -o.astype(np.float32))
    assert np.all(r["tmin"] == np.float32(0.001)) and np.array_equal(r["tmax"], np.arange(5, dtype=np.float32))
    assert sp.make_rays(np.zeros((0, 3)), np.zeros((0, 3))).shape == (0,)
    with pytest.raises(ValueError):
        sp.make_rays(np.zeros((2, 3)), np.zeros((3, 3)))
