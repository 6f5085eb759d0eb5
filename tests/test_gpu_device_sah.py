"""The device SAH builder on the GPU (sp_sah_build.hip; upload(builder="device_sah"); DESIGN.md
section 22).  The acceptance test is equality with the host builder, which is the oracle:

  * the tree read back from the device is the host SAH tree byte for byte (hash over nodes and
    primitive order) on every constructed set of tests/_lbvh_sets.py and tests/_sah_sets.py and on
    bunny.sp, at the default hand-over size and with it lowered so the level kernels run down to
    nodes of a few slots; so are the 8-wide tree and the records under both finishes;
  * images of device-SAH scenes equal the host-built scenes' in every bit, with equal counts, on
    every walk -- the wedge strip on the 8-wide walk included, which the linear BVH cannot pass;
  * a refit of a device-SAH scene gives the refitted host-built scene's arrays and image;
  * the hook, residency and progress objects; bounds that are not finite are refused."""
import os

import numpy as np
import pytest

import simplepath_amd as sp
from simplepath_amd import _abi
from tests import _lbvh_sets, _oracle, _refit_moves as R, _sah_sets

pytestmark = pytest.mark.gpu

REL_L2_TOL = 1e-4
LBVH_SETS = [f"tri{n}" for n in _lbvh_sets.SIZES] + ["identical37", "half_dup", "planar", "collinear", "mixed",
                                                     "spheres_only", "wedge_strip"]
SET_NAMES = LBVH_SETS + list(_sah_sets.NEW)
TREE = ("hash", "nodes", "leaves", "depth", "slots", "max_leaf")
WIDE = ("hash_nodes", "hash_records", "hash_parents")


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    return _sah_sets.write_all(str(tmp_path_factory.mktemp("sah_sets")))


def load(path, w=None, h=None, **upload_options):
    s = sp.Scene.from_file(path)
    if w:
        s.set_resolution(w, h)
    s.upload(device=0, **upload_options)
    return s


def counts(st):
    return (st.rays, st.shadow_rays, st.samples, st.rng_draws, st.stack_depth, st.pipeline)


def same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------- device tree == host SAH tree
def check_tree(s, leaf):
    dev = s.bvh_check()
    host = s.bvh_build_check(builder="host", sah_leaf=leaf)
    assert dev["errors"] == 0 and host["errors"] == 0, (dev, host)
    assert dev["builder"] == "device_sah"
    for k in TREE:
        assert dev[k] == host[k], (k, dev, host)
    info = s.bvh_info()
    assert (info["depth"], info["nodes"], info["slots"]) == (dev["depth"], dev["nodes"], dev["slots"])
    return dev


@pytest.mark.parametrize("leaf", [1, 4])
@pytest.mark.parametrize("name", SET_NAMES + ["bunny"])
def test_device_tree_equals_the_host_tree(sets, scene_dir, name, leaf):
    path = os.path.join(scene_dir, "bunny.sp") if name == "bunny" else sets[name][0]
    s = sp.Scene.from_file(path)
    hashes = {}
    for finish in ("device", "host"):
        s.upload(device=0, builder="device_sah", finish=finish, sah_leaf=leaf)
        dev = check_tree(s, leaf)
        wide = s.wide_check()
        built = s.wide_build_check(builder="host", finish=finish, sah_leaf=leaf)
        print(name, leaf, finish, dev, wide)
        assert wide["errors"] == 0 and wide["finish"] == finish
        for k in WIDE:
            assert wide[k] == built[k], (k, finish, wide, built)
        hashes[finish] = dev["hash"]
    # a second build (the host builder in between forces it) gives the same tree
    s.upload(device=0, builder="host", sah_leaf=leaf)
    mid = s.bvh_check()
    assert mid["builder"] == "host" and mid["errors"] == 0 and mid["hash"] == hashes["device"]
    s.upload(device=0, builder="device_sah", sah_leaf=leaf)
    again = s.bvh_check()
    assert again["builder"] == "device_sah" and again["hash"] == hashes["device"] == hashes["host"]


@pytest.mark.parametrize("small", [4, 37, 1024])
@pytest.mark.parametrize("name", SET_NAMES + ["bunny"])
def test_level_kernels_down_to_small_nodes(sets, scene_dir, monkeypatch, name, small):
    # the hand-over size does not reach the tree: with it lowered, workgroups lie across many open
    # nodes and every split down to a few slots is made by the level kernels; with it raised, one
    # thread builds ranges of up to 1024
    monkeypatch.setenv("SP_SAH_SMALL", str(small))
    path = os.path.join(scene_dir, "bunny.sp") if name == "bunny" else sets[name][0]
    for leaf in (1, 4):
        s = load(path, builder="device_sah", sah_leaf=leaf)
        check_tree(s, leaf)
        assert s.wide_check()["errors"] == 0


# ---------------------------------------------------------------- images: equal to the host build's
@pytest.mark.parametrize("options", [dict(), dict(wide_bvh=False), dict(binary_closest=True), dict(stackless=True)],
                         ids=["default", "binary", "binary_closest", "stackless"])
@pytest.mark.parametrize("scene,w,h,integrator,spp", [
    ("bunny.sp", 64, 40, "direct_lighting", 4),
    ("elf_small.sp", 40, 56, "iterative_rrnee", 2),
    ("lucy_small.sp", 40, 56, "direct_lighting", 4),
])
def test_images_equal_the_host_builds(scene_dir, scene, w, h, integrator, spp, options):
    path = os.path.join(scene_dir, scene)
    dev = load(path, w, h, builder="device_sah", **options)
    assert dev.bvh_check()["builder"] == "device_sah"
    g, gst = sp.render_tiles(dev, integrator, spp)
    host = load(path, w, h, builder="host", **options)
    hg, hst = sp.render_tiles(host, integrator, spp)
    print(scene, options, counts(gst), counts(hst))
    assert counts(gst) == counts(hst)
    assert same_bits(g, hg)
    assert g.max() > 0.0


def test_image_against_the_oracle(scene_dir):
    # DESIGN.md section 1's SAH bar, through the new builder
    path, w, h, integrator, spp = os.path.join(scene_dir, "bunny.sp"), 64, 40, "direct_lighting", 4
    s = load(path, w, h, builder="device_sah")
    g, gst = sp.render_tiles(s, integrator, spp)
    o = sp.Scene.from_file(path)
    o.set_resolution(w, h)
    c, cst = _oracle.render(o, sp.string_to_integrator_type(integrator), spp, variant="spm")
    r = float(np.linalg.norm((g - c).ravel()) / max(np.linalg.norm(c.ravel()), 1e-30))
    frac = float(np.mean(np.all(g == c, axis=-1)))
    print(f"rel_l2={r:.3e} bitexact_pixels={frac:.5f} rays {gst.rays} {cst['rays']}")
    assert r < REL_L2_TOL and frac > 0.999, (r, frac)
    assert gst.rays == cst["rays"] and gst.shadow_rays == cst["shadow_rays"]


@pytest.mark.parametrize("integrator,spp", [("direct_lighting", 3), ("iterative_rrnee", 2)])
def test_wedge_strip_on_the_wide_walk(sets, integrator, spp):
    # the default 8-wide walk: the host SAH tree separates the strip's scales, the linear BVH does
    # not; the device SAH tree is the host's, and so is its image
    path = sets["wedge_strip"][0]
    dev = load(path, 48, 40, builder="device_sah")
    assert dev.bvh_check()["builder"] == "device_sah" and dev.wide_check()["records"] > 0
    g, gst = sp.render_tiles(dev, integrator, spp)
    host = load(path, 48, 40, builder="host")
    hg, hst = sp.render_tiles(host, integrator, spp)
    assert counts(gst) == counts(hst) and gst.stack_depth > 0
    assert same_bits(g, hg)
    assert g.max() > 0.0


# ---------------------------------------------------------------- refit
@pytest.mark.parametrize("name,move", [("tri1025", "jitter"), ("mixed", "shift")])
def test_refit_of_a_device_sah_scene(sets, name, move):
    path = sets[name][0]
    dev = load(path, 48, 40, builder="device_sah")
    v, f = R.mesh_of(dev)
    moved = R.MOVES[move](v, f)
    assert dev.update_mesh(moved, stats=True)["refitted"] == 1
    b, w = dev.bvh_check(), dev.wide_check()
    hb, hw = sp.Scene.from_file(path).refit_build_check(moved, builder="host")
    assert b["errors"] == 0 and w["errors"] == 0
    for k in TREE:
        assert b[k] == hb[k], (k, b, hb)
    for k in WIDE:  # (the finish differs between the two, its bytes do not)
        assert w[k] == hw[k], (k, w, hw)
    host = load(path, 48, 40, builder="host")
    host.update_mesh(moved)
    g, gst = sp.render_tiles(dev, "direct_lighting", 3)
    hg, hst = sp.render_tiles(host, "direct_lighting", 3)
    assert counts(gst) == counts(hst)
    assert same_bits(g, hg)


# ---------------------------------------------------------------- hook, residency, progress objects
def test_env_hook_selects_the_device_sah_builder(scene_dir, monkeypatch):
    monkeypatch.setenv("SP_DEVICE_BUILD", "2")
    s = load(os.path.join(scene_dir, "bunny.sp"))
    assert s.bvh_check()["builder"] == "device_sah" and s.wide_check()["finish"] == "device"
    s.upload(device=0, bvh_mode=1)
    assert s.bvh_check()["builder"] == "host"
    s.upload(device=0, builder="host")
    assert s.bvh_check()["builder"] == "host"


def test_another_builder_invalidates_progress_objects(scene_dir):
    s = load(os.path.join(scene_dir, "bunny.sp"), 32, 24, builder="device")
    for builder in ("device_sah", "host", "device_sah"):
        prog = sp.Progressive(s, "direct_lighting")
        prog.render(1)
        s.upload(device=0, builder=builder)
        with pytest.raises(sp.SimplePathError) as e:
            prog.render(1)
        assert e.value.code == _abi.SP_ERR_STATE
        prog.close()
        assert s.bvh_check()["builder"] == builder
    prog = sp.Progressive(s, "direct_lighting")
    prog.render(1)
    s.upload(device=0, builder="device_sah")  # same options: still resident, still valid
    prog.render(1)
    prog.close()


def test_progress_two_passes_equal_one(scene_dir):
    s = load(os.path.join(scene_dir, "bunny.sp"), 64, 40, builder="device_sah")
    one, _ = sp.render_tiles(s, "direct_lighting", 4)
    prog = sp.Progressive(s, "direct_lighting")
    prog.render(1)
    two, _ = prog.render(3)
    prog.close()
    assert same_bits(one, two)


def test_bounds_that_are_not_finite_are_refused(sets):
    # an infinite vertex passes the loader; its bound has a NaN centroid.  The device SAH builder
    # finds it in its first pass: SP_ERR_UNSUPPORTED, and no resident scene is left behind
    first = sp.Scene.from_file(sets["tri1281"][0])
    v, f = R.mesh_of(first)
    v[700, 1] = np.float32(np.inf)
    s = R.moved_scene(first, v)
    s.upload(device=0, builder="host")
    assert s.bvh_check()["builder"] == "host"
    with pytest.raises(sp.SimplePathError) as e:
        s.upload(device=0, builder="device_sah")
    assert e.value.code == _abi.SP_ERR_UNSUPPORTED
    with pytest.raises(sp.SimplePathError) as e:
        s.bvh_check()
    assert e.value.code == _abi.SP_ERR_STATE
    s.upload(device=0, builder="host")  # and the scene can be uploaded again
    assert s.bvh_check()["errors"] == 0
