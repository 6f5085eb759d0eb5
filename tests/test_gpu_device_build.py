"""The device BVH builder on the GPU (sp_build.hip; upload(builder="device")).

  * The tree the device builds is the tree of its host restatement, bit for bit (hash over nodes
    and primitive order), on every constructed set of tests/_lbvh_sets.py and on bunny.sp, and it
    passes the structural checker after being read back from the device.
  * Images of device-built scenes against the CPU oracle: DESIGN.md §1's SAH bar (rel L2 < 1e-4,
    > 99.9 % of pixels bit-exact: another visiting order can only change which of two primitives
    at exactly equal distance wins) with equal ray counts, and bit-exact on constructed scenes that
    have no such ties or whose ties cannot show.
  * The walks a device-built tree can take (binary, 8-wide, parent links) and progress objects."""
import os

import numpy as np
import pytest

import simplepath_amd as sp
from simplepath_amd import _abi
from tests import _lbvh_sets, _oracle

pytestmark = pytest.mark.gpu

REL_L2_TOL = 1e-4
SET_NAMES = [f"tri{n}" for n in _lbvh_sets.SIZES] + ["identical37", "half_dup", "planar", "collinear", "mixed",
                                                      "spheres_only", "wedge_strip"]


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    return _lbvh_sets.write_all(str(tmp_path_factory.mktemp("lbvh_sets")))


_oracle_cache = {}


def oracle(path, w, h, integrator, spp):
    """the oracle's image and counts of one scene file, computed once"""
    key = (path, w, h, integrator, spp)
    if key not in _oracle_cache:
        s = sp.Scene.from_file(path)
        s.set_resolution(w, h)
        img, st = _oracle.render(s, sp.string_to_integrator_type(integrator), spp, variant="spm")
        img.setflags(write=False)
        _oracle_cache[key] = (img, st)
    return _oracle_cache[key]


def rel_l2(a, b):
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-30))


def within_sah_bar(g, c):
    r, frac = rel_l2(g, c), float(np.mean(np.all(g == c, axis=-1)))
    print(f"rel_l2={r:.3e} bitexact_pixels={frac:.5f}")
    assert r < REL_L2_TOL and frac > 0.999, (r, frac)


def load(path, w=None, h=None, **upload_options):
    s = sp.Scene.from_file(path)
    if w:
        s.set_resolution(w, h)
    s.upload(device=0, **upload_options)
    return s


# ---------------------------------------------------------------- device tree == host restatement
@pytest.mark.parametrize("leaf", [1, 4])
@pytest.mark.parametrize("name", SET_NAMES + ["bunny"])
def test_device_tree_equals_host_restatement(sets, scene_dir, name, leaf):
    path = os.path.join(scene_dir, "bunny.sp") if name == "bunny" else sets[name][0]
    s = load(path, builder="device", sah_leaf=leaf)
    dev = s.bvh_check()
    host = s.bvh_build_check(builder="device", sah_leaf=leaf)
    print(name, leaf, dev)
    assert dev["errors"] == 0 and host["errors"] == 0, (dev, host)
    assert dev["builder"] == "device"
    for k in ("hash", "nodes", "leaves", "depth", "slots", "max_leaf"):
        assert dev[k] == host[k], (k, dev, host)
    info = s.bvh_info()
    assert (info["depth"], info["nodes"], info["slots"]) == (dev["depth"], dev["nodes"], dev["slots"])
    # a second build (the host builder in between forces it) gives the same tree
    s.upload(device=0, builder="host", sah_leaf=leaf)
    mid = s.bvh_check()
    assert mid["builder"] == "host" and mid["errors"] == 0
    assert mid["hash"] == s.bvh_build_check(builder="host", sah_leaf=leaf)["hash"]
    s.upload(device=0, builder="device", sah_leaf=leaf)
    assert s.bvh_check()["hash"] == dev["hash"]


def test_reference_order_upload_passes_the_checker(scene_dir):
    s = load(os.path.join(scene_dir, "bunny.sp"), bvh_mode=1)
    c = s.bvh_check()
    assert c["errors"] == 0 and c["builder"] == "host"
    assert c["hash"] == s.bvh_build_check(bvh_mode=1)["hash"]


def test_env_hook_selects_the_device_builder(scene_dir, monkeypatch):
    monkeypatch.setenv("SP_DEVICE_BUILD", "1")
    s = load(os.path.join(scene_dir, "bunny.sp"))
    assert s.bvh_check()["builder"] == "device"
    s.upload(device=0, bvh_mode=1)
    assert s.bvh_check()["builder"] == "host"


# ---------------------------------------------------------------- images against the oracle
@pytest.mark.parametrize("scene,w,h,integrator,spp", [
    ("bunny.sp", 64, 40, "direct_lighting", 4),
    ("lucy_small.sp", 40, 56, "direct_lighting", 4),
    ("elf_small.sp", 40, 56, "direct_lighting", 4),
    ("elf_small.sp", 40, 56, "iterative_rrnee", 2),
])
def test_image_parity_against_the_oracle(scene_dir, scene, w, h, integrator, spp):
    path = os.path.join(scene_dir, scene)
    s = load(path, w, h, builder="device")
    assert s.bvh_check()["builder"] == "device"
    g, gst = sp.render_tiles(s, integrator, spp)
    c, cst = oracle(path, w, h, integrator, spp)
    print(scene, integrator, "rays", gst.rays, cst["rays"], "shadow", gst.shadow_rays, cst["shadow_rays"])
    within_sah_bar(g, c)
    assert gst.rays == cst["rays"] and gst.shadow_rays == cst["shadow_rays"]


@pytest.mark.parametrize("name", ["tri257", "identical37"])
@pytest.mark.parametrize("integrator,spp", [("direct_lighting", 3), ("iterative_rrnee", 2)])
def test_constructed_scenes_bit_exact(sets, name, integrator, spp):
    # separated triangles: no two primitives at one distance along any ray; identical triangles:
    # every ray ties, and every copy gives the same record
    path = sets[name][0]
    s = load(path, 48, 40, builder="device")
    chk = s.bvh_check()
    assert chk["builder"] == "device" and chk["errors"] == 0
    g, gst = sp.render_tiles(s, integrator, spp)
    c, cst = oracle(path, 48, 40, integrator, spp)
    diff = np.argwhere(np.any(g.view(np.uint32) != c.view(np.uint32), axis=-1))
    print(name, integrator, "depth", chk["depth"], "differing pixels", diff[:8].tolist())
    assert gst.rays == cst["rays"] and gst.shadow_rays == cst["shadow_rays"]
    assert diff.size == 0, (name, rel_l2(g, c), diff[:8].tolist())


@pytest.mark.parametrize("walk", ["stackless", "binary"])
@pytest.mark.parametrize("integrator,spp", [("direct_lighting", 3), ("iterative_rrnee", 2)])
def test_wedge_strip_bit_exact(sets, walk, integrator, spp):
    # The strip's largest triangles overflow the triangle test's products (edges of 4e19 and more):
    # tri_hit, like the reference's test, then reports a hit at t = NaN for any ray that reaches
    # it, so the image is the oracle's only while no walk tests a triangle whose exact box the ray
    # misses.  The binary walks test exact boxes.  The 8-wide nodes' boxes are quantised outward on
    # a grid of 1/254 of a node's extent; in the linear BVH most of the strip shares one Morton
    # cell and is grouped by position, so one wide node spans many orders of magnitude and its
    # grid reaches such triangles (measured: 1480 of 1920 pixels differ; the host SAH tree, which
    # separates the scales, does not show it).  So the strip is walked deep
    # (binary) or, with a stack budget below the tree's depth, without a stack: also a binary walk.
    path = sets["wedge_strip"][0]
    depth = sp.Scene.from_file(path).bvh_build_check(builder="device")["depth"]
    assert depth >= 8
    options = dict(stack_max_levels=depth - 2) if walk == "stackless" else dict(wide_bvh=False)
    s = load(path, 48, 40, builder="device", **options)
    chk = s.bvh_check()
    assert chk["builder"] == "device" and chk["errors"] == 0 and chk["depth"] == depth
    g, gst = sp.render_tiles(s, integrator, spp)
    assert (gst.stack_depth == 0) == (walk == "stackless")
    c, cst = oracle(path, 48, 40, integrator, spp)
    diff = np.argwhere(np.any(g.view(np.uint32) != c.view(np.uint32), axis=-1))
    print("wedge_strip", walk, integrator, "depth", depth, "differing pixels", diff[:8].tolist())
    assert gst.rays == cst["rays"] and gst.shadow_rays == cst["shadow_rays"]
    assert diff.size == 0, (rel_l2(g, c), diff[:8].tolist())
    assert g.max() > 0.0


# ---------------------------------------------------------------- the walks, progress objects
@pytest.mark.parametrize("options", [dict(wide_bvh=False), dict(binary_closest=True), dict(stackless=True)],
                         ids=["binary", "binary_closest", "stackless"])
def test_walks_on_a_device_built_tree(scene_dir, options):
    path = os.path.join(scene_dir, "bunny.sp")
    c, cst = oracle(path, 64, 40, "direct_lighting", 4)
    dev = load(path, 64, 40, builder="device", **options)
    g, gst = sp.render_tiles(dev, "direct_lighting", 4)
    host = load(path, 64, 40, builder="host", **options)
    hg, hst = sp.render_tiles(host, "direct_lighting", 4)
    for img in (g, hg):
        assert rel_l2(img, c) < REL_L2_TOL
    frac = float(np.mean(np.all(g == hg, axis=-1)))
    print(options, "device vs host SAH: equal pixels", frac, "rays", gst.rays, hst.rays, cst["rays"])
    assert frac > 0.999


def test_progress_two_passes_equal_one(scene_dir):
    s = load(os.path.join(scene_dir, "bunny.sp"), 64, 40, builder="device")
    one, _ = sp.render_tiles(s, "direct_lighting", 4)
    prog = sp.Progressive(s, "direct_lighting")
    prog.render(1)
    two, _ = prog.render(3)
    prog.close()
    assert np.array_equal(one.view(np.uint32), two.view(np.uint32))


def test_another_builder_invalidates_progress_objects(scene_dir):
    s = load(os.path.join(scene_dir, "bunny.sp"), 32, 24, builder="device")
    prog = sp.Progressive(s, "direct_lighting")
    prog.render(1)
    s.upload(device=0, builder="device")  # same options: still resident, still valid
    prog.render(1)
    s.upload(device=0, builder="host")
    with pytest.raises(sp.SimplePathError) as e:
        prog.render(1)
    assert e.value.code == _abi.SP_ERR_STATE
    prog.close()
    prog = sp.Progressive(s, "direct_lighting")
    prog.render(1)
    s.upload(device=0, builder="device")
    with pytest.raises(sp.SimplePathError) as e:
        prog.render(1)
    assert e.value.code == _abi.SP_ERR_STATE
    prog.close()
