"""Pin the CPU oracle to the reference itself.

oracle/_ref/libsp_ref.so is the reference's render path compiled from the sources under
/root/reference (oracle/build_ref.sh + oracle/ref_harness.cpp): the reference's own Scene,
BVHAccelerator, shapes, materials, lights, samplers and integrators, driven by main.cpp's
per-pixel loop.  The C oracle built against glibc's float libm (liboracle_glibc.so: reference
semantics) must reproduce it bit for bit; the GPU is in turn checked bit-exact against the oracle
(tests/test_gpu_parity.py), closing the chain reference == oracle == HIP path.

The library exists only where the reference sources were available at build time.  Its output for
every case below is stored in tests/golden/ref_tiles.npz (written by this module with
SP_WRITE_REF_GOLDEN=1 where the library exists), so elsewhere the oracle is checked against those
recorded tiles; where the library exists it renders again and, on a CPU like the record's, must
also reproduce the record (class Ref).
"""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import simplepath_amd as sp
from tests import _oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libsp_ref.so")


GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_tiles.npz")
WRITE_GOLDEN = os.environ.get("SP_WRITE_REF_GOLDEN") == "1"


class Ref:
    """The reference's tiles: rendered by oracle/_ref/libsp_ref.so where it is built (and equal to
    the record), read from the record elsewhere.

    The reference normalises with RSQRTSS, whose results differ between CPU vendors, so the record
    carries the RSQRTSS table of the CPU it was rendered on (as tests/golden/*_full_tiles.npz do).
    The device path can emulate that CPU (recorded_cpu()); the C oracle executes the instruction,
    so without the library it can be checked against the record only on a CPU with the same table."""

    def __init__(self, lib):
        self.lib = lib
        self.golden = dict(np.load(GOLDEN)) if os.path.exists(GOLDEN) and not WRITE_GOLDEN else {}
        self.rendered = {}
        self.host = sp.rsqrt_table()
        self.same_cpu = bool(self.golden) and \
            (int(self.golden["rsqrt_bits"]), int(self.golden["rsqrt_zero"]), int(self.golden["rsqrt_denorm"])) == \
            (self.host["bits"], self.host["zero_result"], self.host["denorm_result"]) and \
            np.array_equal(self.golden["rsqrt_entries"], self.host["entries"])

    @contextlib.contextmanager
    def recorded_cpu(self):
        """Scenes built and rendered by simplepath_amd inside this block use the RSQRTSS of the CPU
        the tiles render() returns come from: this host's with the library, else the record's."""
        if self.lib is not None or self.same_cpu:
            yield
            return
        g = self.golden
        sp.set_rsqrt_table({"entries": g["rsqrt_entries"], "bits": int(g["rsqrt_bits"]),
                            "zero_result": int(g["rsqrt_zero"]), "denorm_result": int(g["rsqrt_denorm"])})
        try:
            yield
        finally:
            sp.set_rsqrt_table(None)

    def render(self, path, w, h, integrator, spp, ids, host_rsqrt=True):
        """host_rsqrt: the caller compares with code that executes this host's RSQRTSS (the oracle)."""
        key = f"{os.path.basename(path)}_{w}x{h}_i{integrator}_s{spp}_n{ids.size}"
        if self.lib is None:
            if host_rsqrt and not self.same_cpu:
                pytest.skip("oracle/_ref is not built here and its recorded tiles come from a CPU with another RSQRTSS")
            return self.golden[key].view(np.float32)
        out = np.zeros((ids.size, 64, 3), dtype=np.float32)
        rc = self.lib.ref_render(path.encode(), w, h, integrator, spp, ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                 ids.size, 8, out.ctypes.data_as(C.POINTER(C.c_float)))
        assert rc == 0, self.lib.ref_last_error()
        if WRITE_GOLDEN:
            self.rendered[key] = out.view(np.uint32)  # bit patterns: the map's infinities and NaNs survive
        elif self.same_cpu:
            assert np.array_equal(out.view(np.uint32), self.golden[key]), f"{key}: the record is stale"
        return out

    def save(self):
        t = self.host
        np.savez_compressed(GOLDEN, rsqrt_entries=t["entries"], rsqrt_bits=t["bits"], rsqrt_zero=t["zero_result"],
                            rsqrt_denorm=t["denorm_result"], **self.rendered)


def open_ref():
    if not os.path.exists(REF_LIB):
        if os.path.isdir("/root/reference"):
            import subprocess
            subprocess.run(["bash", os.path.join(ROOT, "oracle", "build_ref.sh")], check=True, timeout=1200)
    L = None
    if os.path.exists(REF_LIB):
        L = C.CDLL(REF_LIB)
        L.ref_render.restype = C.c_int
        L.ref_render.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_uint32, C.POINTER(C.c_int32), C.c_int64,
                                 C.c_int, C.POINTER(C.c_float)]
        L.ref_last_error.restype = C.c_char_p
    return Ref(L)


@pytest.fixture(scope="module")
def ref():
    r = open_ref()
    yield r
    if WRITE_GOLDEN and r.rendered:
        r.save()


def ref_render(L, path, w, h, integrator, spp, ids, host_rsqrt=True):
    return L.render(path, w, h, integrator, spp, np.ascontiguousarray(ids, dtype=np.int32), host_rsqrt)


def oracle_render(path, w, h, integrator, spp, ids):
    s = sp.Scene.from_file(path)
    s.set_resolution(w, h)
    out, _ = _oracle.render(s, integrator, spp, ids, variant="glibc")
    return out


def same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_bunny_direct_lighting(ref, scene_dir):
    path = os.path.join(scene_dir, "bunny.sp")
    ids = np.arange(sp.TileScheduler(64, 40).get_num_tiles(), dtype=np.int32)
    r = ref_render(ref, path, 64, 40, 6, 4, ids)
    o = oracle_render(path, 64, 40, 6, 4, ids)
    assert same(r, o), float(np.abs(r - o).max())
    assert r.max() > 0.0


def test_bunny_clipped_tiles_and_order(ref, scene_dir):
    path = os.path.join(scene_dir, "bunny.sp")
    n = sp.TileScheduler(70, 35).get_num_tiles()
    ids = np.array([n - 1, 3, 0, n // 2], dtype=np.int32)  # ragged border tiles, any order
    r = ref_render(ref, path, 70, 35, 6, 3, ids)
    o = oracle_render(path, 70, 35, 6, 3, ids)
    assert same(r, o)


@pytest.mark.parametrize("integrator", ["direct_lighting", "brute_force", "brute_force_iterative",
                                        "brute_force_iterative_rr", "iterative_rrnee", "whitted", "mandelbrot"])
def test_spheres_every_integrator(ref, scene_dir, integrator):
    path = os.path.join(scene_dir, "material_spheres.sp")
    t = sp.string_to_integrator_type(integrator)
    ids = np.arange(sp.TileScheduler(24, 48).get_num_tiles(), dtype=np.int32)
    r = ref_render(ref, path, 24, 48, t, 3, ids)
    o = oracle_render(path, 24, 48, t, 3, ids)
    assert same(r, o), (integrator, float(np.abs(r - o).max()))


def test_bunny_multibounce(ref, scene_dir):
    path = os.path.join(scene_dir, "bunny.sp")
    ids = np.arange(0, sp.TileScheduler(32, 24).get_num_tiles(), dtype=np.int32)
    r = ref_render(ref, path, 32, 24, 5, 2, ids)
    o = oracle_render(path, 32, 24, 5, 2, ids)
    assert same(r, o)


@pytest.mark.parametrize("integrator", ["direct_lighting", "brute_force_iterative_rr", "iterative_rrnee", "whitted",
                                        "brute_force"])
def test_image_environment_light(ref, scene_dir, integrator):
    """scenes/material_spheres.sp with its ImageBasedEnvironmentLight (synthetic HDR map with
    clamped, infinite, negative and black texels): light sampling through Distribution2D,
    the light pdf of the MIS integrator, and radiance lookups of escaping rays."""
    path = os.path.join(scene_dir, "material_spheres_ibl.sp")
    t = sp.string_to_integrator_type(integrator)
    ids = np.arange(sp.TileScheduler(24, 48).get_num_tiles(), dtype=np.int32)
    r = ref_render(ref, path, 24, 48, t, 4, ids)
    o = oracle_render(path, 24, 48, t, 4, ids)
    assert same(r, o), (integrator, float(np.abs(r - o).max()), int(np.sum(r != o)))
    assert r.max() > 0.0


@pytest.mark.parametrize("scene,integrator,spp", [("bunny_scan.sp", "direct_lighting", 3),
                                                  ("lucy_small.sp", "direct_lighting", 3),
                                                  ("elf_small.sp", "direct_lighting", 3),
                                                  ("elf_small.sp", "iterative_rrnee", 2)])
def test_figure_scenes(ref, scene_dir, scene, integrator, spp):
    """lucy.sp (PLY with a scene rotation) and elf.sp (binary STL: std::map vertex welding,
    file face normals; max_depth 16) with their constant environment lights."""
    path = os.path.join(scene_dir, scene)
    t = sp.string_to_integrator_type(integrator)
    ids = np.arange(sp.TileScheduler(40, 56).get_num_tiles(), dtype=np.int32)
    r = ref_render(ref, path, 40, 56, t, spp, ids)
    o = oracle_render(path, 40, 56, t, spp, ids)
    assert same(r, o), (scene, integrator, float(np.abs(r - o).max()))
    assert r.max() > 0.0


@pytest.mark.parametrize("scene,w,h,integrator,spp", [("bunny.sp", 32, 24, "iterative_rrnee", 2),
                                                      ("material_spheres_ibl.sp", 24, 48, "iterative_rrnee", 3)])
def test_device_parity_cases(ref, scene_dir, scene, w, h, integrator, spp):
    """The cases of tests/test_gpu_parity.py::test_vs_reference_build_bitexact that no test above
    renders: the device test reads them from the same record where the library is not built."""
    path = os.path.join(scene_dir, scene)
    t = sp.string_to_integrator_type(integrator)
    ids = np.arange(sp.TileScheduler(w, h).get_num_tiles(), dtype=np.int32)
    r = ref_render(ref, path, w, h, t, spp, ids)
    o = oracle_render(path, w, h, t, spp, ids)
    assert same(r, o), (scene, integrator, float(np.abs(r - o).max()))
    assert r.max() > 0.0


@pytest.mark.parametrize("integrator", ["brute_force", "whitted", "iterative_rrnee"])
def test_deep_recursion(ref, scene_dir, integrator):
    """Closed room, max_depth 40: recursive paths run to the depth limit."""
    path = os.path.join(scene_dir, "closed_room.sp")
    t = sp.string_to_integrator_type(integrator)
    ids = np.arange(sp.TileScheduler(16, 16).get_num_tiles(), dtype=np.int32)
    r = ref_render(ref, path, 16, 16, t, 2, ids)
    o = oracle_render(path, 16, 16, t, 2, ids)
    assert same(r, o), (integrator, float(np.abs(r - o).max()))
    assert r.max() > 0.0


@pytest.mark.parametrize("integrator", ["direct_lighting", "iterative_rrnee"])
def test_degenerate_deep_bvh(ref, scene_dir, integrator):
    """A wedge strip whose reference BVH nests 172 levels (shapes/BVHAccelerator.h:62-77 recurses
    without bound): the oracle's recursive walk and the reference agree bit for bit."""
    path = os.path.join(scene_dir, "wedge_strip.sp")
    t = sp.string_to_integrator_type(integrator)
    ids = np.arange(sp.TileScheduler(64, 48).get_num_tiles(), dtype=np.int32)
    r = ref_render(ref, path, 64, 48, t, 3, ids)
    o = oracle_render(path, 64, 48, t, 3, ids)
    assert same(r, o), (integrator, float(np.abs(r - o).max()))
    assert r.max() > 0.0
