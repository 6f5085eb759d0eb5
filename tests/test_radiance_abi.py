"""sp_scene_radiance_rays without a device (include/simplepath_hip.h, "radiance queries"): the
announcement in the header, the layout of sp_radiance_ray and sp_radiance_query in C, ctypes and
numpy, every refusal in the order the header states on a scene that is not resident -- so the
residency check, which comes last of them, answers only once everything before it is in order --,
pixel_seed and the records make_radiance_rays writes."""
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
ARG, STATE = _abi.SP_ERR_ARG, _abi.SP_ERR_STATE
ALIGNED, ODD = 0x1000, 0x1008  # stand-in device addresses: validation never reads through them
FIELDS = ("integrator", "d_rays", "num_rays", "samples_per_ray", "waves_per_simd", "flags", "reserved0", "stream", "reserved")
RAY_FIELDS = ("o", "seed", "d", "reserved")


def test_header_announces_the_surface():
    src = open(HEADER).read()
    assert re.search(r"^#define SP_HAS_RADIANCE_QUERY 1\b", src, re.M)
    assert re.search(r"#define SP_ABI_VERSION 6\b", src)  # new entry points only
    for name in ("sp_scene_radiance_rays", "sp_scene_radiance_rays_host"):
        assert re.search(r"\b%s\(" % name, src), name
        assert name in _abi.SIGNATURES and hasattr(sp.lib(), name), name
    for name in ("RADIANCE_RAY_DTYPE", "make_radiance_rays", "pixel_seed"):
        assert name in sp.__all__
    assert hasattr(sp.Scene, "radiance") and hasattr(sp.Scene, "radiance_device")
    # what a caller has to know, stated where a caller reads it
    for words in ("caller normalises", "correlated noise", "0xb0ae9d99", "does not depend on its position"):
        assert words in src, words


def test_struct_layouts_match_the_compiler(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "simplepath_hip.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(sp_radiance_query));\n'
                   + "".join('  printf(" %%zu", offsetof(sp_radiance_query, %s));\n' % f for f in FIELDS)
                   + '  printf("\\n%zu", sizeof(sp_radiance_ray));\n'
                   + "".join('  printf(" %%zu", offsetof(sp_radiance_ray, %s));\n' % f for f in RAY_FIELDS)
                   + '  printf("\\n");\n  return SP_HAS_RADIANCE_QUERY == 1 ? 0 : 1;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, timeout=120)
    a, b = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.splitlines()
    Q, R = _abi.sp_radiance_query, _abi.sp_radiance_ray
    assert [name for name, _ in Q._fields_] == ["struct_size", *FIELDS]
    # no implicit padding: every field starts where the one before it ends
    assert [int(x) for x in a.split()] == [C.sizeof(Q)] + [getattr(Q, f).offset for f in FIELDS] \
        == [64, 4, 8, 16, 24, 28, 32, 36, 40, 48]
    assert [int(x) for x in b.split()] == [C.sizeof(R)] + [getattr(R, f).offset for f in RAY_FIELDS] == [32, 0, 12, 16, 28]
    D = sp.RADIANCE_RAY_DTYPE
    assert D.itemsize == 32 and [D.fields[f][1] for f in RAY_FIELDS] == [0, 12, 16, 28]


def test_pixel_seed():
    assert sp.pixel_seed(0, 0) == 0xb0ae9d99
    assert sp.pixel_seed(3, 5) == ((3 << 16) | 5) ^ 0xb0ae9d99
    assert sp.pixel_seed(65535, 65535) == 0xffffffff ^ 0xb0ae9d99
    x, y = np.meshgrid(np.arange(7), np.arange(4))
    s = sp.pixel_seed(x, y)
    assert s.dtype == np.uint32 and s.shape == (4, 7)
    assert s[2, 6] == sp.pixel_seed(6, 2) and isinstance(sp.pixel_seed(6, 2), int)


def test_make_radiance_rays_layout():
    o = np.arange(6, dtype=np.float64).reshape(2, 3) + 0.5
    d = -np.arange(6, dtype=np.float32).reshape(2, 3) - 1.0
    rays = sp.make_radiance_rays(o, d, [7, 0xfffffffe])
    assert rays.dtype == sp.RADIANCE_RAY_DTYPE and rays.shape == (2,)
    words = rays.view(np.uint32).reshape(2, 8)
    floats = rays.view(np.float32).reshape(2, 8)
    assert np.array_equal(floats[:, 0:3], o.astype(np.float32)) and np.array_equal(floats[:, 4:7], d)
    assert words[:, 3].tolist() == [7, 0xfffffffe] and words[:, 7].tolist() == [0, 0]
    assert sp.make_radiance_rays(o, d, 9)["seed"].tolist() == [9, 9]  # one seed for all
    assert sp.make_radiance_rays(o, d, sp.pixel_seed(np.array([1, 2]), np.array([3, 4])))["seed"].tolist() == \
        [sp.pixel_seed(1, 3), sp.pixel_seed(2, 4)]
    assert sp.make_radiance_rays(np.zeros((0, 3)), np.zeros((0, 3)), []).shape == (0,)
    with pytest.raises(ValueError):
        sp.make_radiance_rays(o, d[:1], 0)


@pytest.fixture(scope="module")
def scene(scene_dir):
    s = sp.Scene.from_file(os.path.join(scene_dir, "bunny.sp"))  # never uploaded
    s.set_resolution(20, 12)
    return s


def query(n=5, rays=ALIGNED, integrator="direct_lighting", samples=2, waves=0, flags=0):
    q = _abi.sp_radiance_query()
    q.struct_size = C.sizeof(q)
    q.integrator = _abi.INTEGRATORS[integrator] if isinstance(integrator, str) else integrator
    q.d_rays = rays or None
    q.num_rays, q.samples_per_ray, q.waves_per_simd, q.flags = n, samples, waves, flags
    return q


def test_refusals_come_in_the_stated_order(scene):
    L = sp.lib()
    OUT = C.c_void_p(ALIGNED)
    call = lambda s, q, out=OUT: L.sp_scene_radiance_rays(s, None if q is None else C.byref(q), out, None)
    err = lambda: L.sp_last_error()
    # everything in order: only the residency is missing
    assert call(scene.handle, query()) == STATE and b"sp_scene_upload" in err()
    assert call(scene.handle, query(flags=sp.PER_LANE_QUERIES, waves=4)) == STATE
    assert call(scene.handle, query(integrator="iterative_rrnee", waves=2)) == STATE
    assert call(scene.handle, query(integrator=0)) == STATE       # not specified: the scene's
    assert call(scene.handle, query(n=0, rays=0)) == STATE        # no rays need no buffer, but a resident scene
    # (what is refused after the residency is not looked at before it)
    assert call(scene.handle, query(integrator="mandelbrot")) == STATE
    assert call(scene.handle, query(integrator=99, waves=9)) == STATE
    assert call(scene.handle, query(n=2 ** 40)) == STATE
    # 1. null scene, query or output -- before anything in the query is looked at
    bad = query()
    bad.struct_size = 0
    assert call(None, bad) == ARG and b"null" in err()
    assert call(scene.handle, None) == ARG and b"null" in err()
    assert call(scene.handle, bad, None) == ARG and b"null" in err()
    # 2. struct_size and reserved words -- before the flags
    q = query(flags=1)
    q.struct_size -= 8
    assert call(scene.handle, q) == ARG and b"struct_size" in err()
    for k in range(5):
        q = query(flags=1)
        if k < 4:
            q.reserved[k] = 1
        else:
            q.reserved0 = 1
        assert call(scene.handle, q) == ARG and b"reserved" in err()
    # 3. flags -- before the ray count
    for flags in (1, 2, 3, 4, 16, sp.PER_LANE_QUERIES | 1, -1):
        assert call(scene.handle, query(n=-1, flags=flags)) == ARG and b"flags" in err()
    # 4. num_rays < 0 -- before the ray buffer
    assert call(scene.handle, query(n=-1, rays=0)) == ARG and b"num_rays" in err()
    # 5. d_rays missing when there are rays, or misaligned (with or without rays) -- before the samples
    assert call(scene.handle, query(rays=0, samples=0)) == ARG and b"d_rays" in err()
    assert call(scene.handle, query(rays=ODD, samples=0)) == ARG and b"aligned" in err()
    assert call(scene.handle, query(n=0, rays=ODD, samples=0)) == ARG and b"aligned" in err()
    # 6. samples_per_ray == 0 -- before the occupancy request
    assert call(scene.handle, query(samples=0, waves=9)) == ARG and b"samples_per_ray" in err()
    # 7. waves_per_simd out of the integrator's range -- before the residency
    for integrator, waves in (("direct_lighting", 5), ("direct_lighting", -1), ("iterative_rrnee", 1), ("whitted", 2),
                              ("brute_force", 4), (0, 5)):
        assert call(scene.handle, query(integrator=integrator, waves=waves)) == ARG and b"waves_per_simd" in err()
    # 8. SP_ERR_STATE is last of them: nothing above was wrong with the first calls


def test_the_host_form_and_the_wrappers_refuse_alike(scene):
    L = sp.lib()
    rays = sp.make_radiance_rays(np.zeros((5, 3)), np.ones((5, 3)), 1)
    out = np.zeros((5, 3), dtype=np.float32)
    host = lambda s, q, r=rays, o=out: L.sp_scene_radiance_rays_host(
        s, None if q is None else C.byref(q), None if r is None else C.c_void_p(r.ctypes.data),
        None if o is None else C.c_void_p(o.ctypes.data), None)
    assert host(None, query()) == ARG
    assert host(scene.handle, None) == ARG
    assert host(scene.handle, query(), rays, None) == ARG
    assert host(scene.handle, query(flags=2)) == ARG
    assert host(scene.handle, query(n=-1)) == ARG
    assert host(scene.handle, query(), None) == ARG and b"h_rays" in L.sp_last_error()
    assert host(scene.handle, query(samples=0)) == ARG
    assert host(scene.handle, query(waves=7)) == ARG
    # d_rays is ignored, and no alignment is asked of the host array
    odd = np.zeros(5 * 8 + 2, dtype=np.uint32)[2:].view(sp.RADIANCE_RAY_DTYPE)  # 8 bytes off the allocation's alignment
    assert host(scene.handle, query(rays=ODD), odd) == STATE
    assert host(scene.handle, query(rays=0)) == STATE
    assert host(scene.handle, query(n=0), None) == STATE
    with pytest.raises(sp.SimplePathError) as e:
        scene.radiance(np.zeros((2, 3)), np.ones((2, 3)), [1, 2], "direct_lighting", 2)
    assert e.value.code == STATE
    with pytest.raises(sp.SimplePathError) as e:
        scene.radiance(np.zeros((2, 3)), np.ones((2, 3)), [1, 2], "direct_lighting", 0)
    assert e.value.code == ARG
    with pytest.raises(sp.SimplePathError) as e:
        scene.radiance_device(ODD, 2, ALIGNED, "direct_lighting", 2)
    assert e.value.code == ARG
    with pytest.raises(sp.SimplePathError) as e:
        scene.radiance_device(ALIGNED, 2, ALIGNED, "direct_lighting", 2, stats=False, per_lane_queries=True)
    assert e.value.code == STATE
