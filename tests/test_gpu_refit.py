"""The device refit on the GPU (sp_refit.hip; Scene.update_mesh on a resident scene).

  * Arrays: after upload(...) and update_mesh(move), the binary tree and the 8-wide tree read back
    from the device pass both structural checkers against the MOVED mesh, and all five hashes equal
    the host restatement's (refit_build_check) -- over constructed sets x deformations x leaf size
    x {host SAH, device LBVH} x {host, device finish}.  The moves are applied one after another to
    one residency: a refit depends on the topology and the new positions alone.
  * Images: a null refit changes no bit and no count; on sets without equal-distance ties the image
    after a refit is the oracle's image of scene.desc(), bit for bit, for every walk; on a bunny,
    where ties are possible, the refitted scene meets the SAH bar that a fresh
    SAH upload of the same moved mesh meets.
  * State: progress objects, re-uploads, refused calls."""
import ctypes as C
import os

import numpy as np
import pytest

import simplepath_amd as sp
from simplepath_amd import _abi
from tests import _lbvh_sets, _oracle, _refit_moves as R

pytestmark = pytest.mark.gpu

W, H = 64, 48
REL_L2_TOL = 1e-4
HASHES = (("b", "hash"), ("w", "hash_nodes"), ("w", "hash_records"), ("w", "hash_parents"))
COUNTS = (("b", "nodes"), ("b", "slots"), ("b", "depth"), ("w", "records"), ("w", "holes"), ("w", "slots"), ("w", "depth"))
INTEGRATORS = (("direct_lighting", 3), ("iterative_rrnee", 2))


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    return _lbvh_sets.write_all(str(tmp_path_factory.mktemp("refit_sets")))


def load(path, upload=True, **upload_options):
    s = sp.Scene.from_file(path)
    s.set_resolution(W, H)
    if upload:
        s.upload(device=0, **upload_options)
    return s


def picked(b, w, keys):
    return tuple({"b": b, "w": w}[which][k] for which, k in keys)


def rel_l2(a, b):
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-30))


def within_sah_bar(g, c):
    r, frac = rel_l2(g, c), float(np.mean(np.all(g == c, axis=-1)))
    print(f"rel_l2={r:.3e} bitexact_pixels={frac:.5f}")
    assert r < REL_L2_TOL and frac > 0.999, (r, frac)


def oracle_of(scene, integrator, spp):
    img, st = _oracle.render(scene, sp.string_to_integrator_type(integrator), spp, variant="spm")
    img.setflags(write=False)
    return img, st


def bit_exact(g, gst, c, cst, what):
    diff = np.argwhere(np.any(g.view(np.uint32) != c.view(np.uint32), axis=-1))
    assert gst.rays == cst["rays"] and gst.shadow_rays == cst["shadow_rays"], (what, gst.rays, cst["rays"])
    assert diff.size == 0, (what, rel_l2(g, c), diff[:8].tolist())


# ---------------------------------------------------------------- arrays and checkers
@pytest.mark.parametrize("name", R.SETS)
def test_refitted_arrays_equal_the_host_restatement(sets, name):
    first = sp.Scene.from_file(sets[name][0])  # keeps pose A: the topology every refit below works on
    v, f = R.mesh_of(first)
    for builder in R.BUILDERS:
        for finish in ("host", "device"):
            for leaf in R.LEAVES:
                opts = dict(builder=builder, finish=finish, sah_leaf=leaf)
                s = load(sets[name][0], **opts)
                info, nbytes = s.bvh_info(), s.device_bytes()
                for move, fn in R.MOVES.items():
                    moved = fn(v, f)
                    st = s.update_mesh(moved, stats=True)
                    assert st["refitted"] == 1 and st["binary_passes"] == max(info["depth"] - 1, 0), (move, st, info)
                    b, w = s.bvh_check(), s.wide_check()
                    hb, hw = first.refit_build_check(moved, **opts)
                    what = (name, builder, finish, leaf, move)
                    assert b["errors"] == 0 and w["errors"] == 0, (what, b, w)
                    assert hb["errors"] == 0 and hw["errors"] == 0, (what, hb, hw)
                    assert picked(b, w, HASHES) == picked(hb, hw, HASHES), (what, b, w, hb, hw)
                    assert picked(b, w, COUNTS) == picked(hb, hw, COUNTS), (what, b, w, hb, hw)
                    assert st["wide_passes"] == max(w["depth"] - 1, 0) and (b["builder"], w["finish"]) == (builder, finish)
                # back at A after all of them: the bytes of A -> A
                s.update_mesh(v)
                hb, hw = first.refit_build_check(v, **opts)
                assert picked(s.bvh_check(), s.wide_check(), HASHES) == picked(hb, hw, HASHES), (name, opts)
                if builder == "device":  # the same fold as the device build's: the binary tree's bytes are the build's
                    assert hb["hash"] == first.bvh_build_check(builder=builder, sah_leaf=leaf)["hash"]
                assert s.bvh_info() == info and s.device_bytes() == nbytes


@pytest.mark.parametrize("options", [dict(stackless=True), dict(wide_bvh=False)], ids=["stackless", "no_wide_bvh"])
def test_scenes_without_a_wide_tree(sets, options):
    for name in ("mixed", "tri257"):
        first = sp.Scene.from_file(sets[name][0])
        v, f = R.mesh_of(first)
        for builder in R.BUILDERS:
            s = load(sets[name][0], builder=builder, **options)
            for move in ("permute", "collapse_half", "shift"):
                moved = R.MOVES[move](v, f)
                st = s.update_mesh(moved, stats=True)
                b, w = s.bvh_check(), s.wide_check()
                hb, hw = first.refit_build_check(moved, builder=builder, **options)
                assert b["errors"] == 0 and w["errors"] == 0, (name, builder, move, b, w)
                assert picked(b, w, HASHES) == picked(hb, hw, HASHES), (name, builder, move)
                assert (w["records"], w["hash_nodes"], st["wide_passes"]) == (0, 0, 0)
                assert (w["hash_parents"] != 0) == ("stackless" in options)


# ---------------------------------------------------------------- images
@pytest.mark.parametrize("builder", R.BUILDERS)
@pytest.mark.parametrize("name", ["tri257", "bunny"])
def test_null_refit_changes_nothing(sets, scene_dir, name, builder):
    path = os.path.join(scene_dir, "bunny.sp") if name == "bunny" else sets[name][0]
    s = load(path, builder=builder)
    v, f = R.mesh_of(s)
    info, nbytes = s.bvh_info(), s.device_bytes()
    before = {i: sp.render_tiles(s, i, spp) for i, spp in INTEGRATORS}
    s.update_mesh(R.identity(v, f))
    for i, spp in INTEGRATORS:
        g, st = sp.render_tiles(s, i, spp)
        g0, st0 = before[i]
        assert (st.rays, st.shadow_rays, st.rng_draws) == (st0.rays, st0.shadow_rays, st0.rng_draws)
        assert np.array_equal(g.view(np.uint32), g0.view(np.uint32))
    assert s.bvh_info() == info and s.device_bytes() == nbytes


WALKS = {"wide": dict(), "binary_closest": dict(binary_closest=True), "no_wide_bvh": dict(wide_bvh=False),
         "stackless": dict(stackless=True)}


@pytest.mark.parametrize("move", R.RENDERED)
@pytest.mark.parametrize("name", ["tri65", "tri1025"])
def test_tie_free_sets_bit_exact_against_the_oracle(sets, name, move):
    # separated triangles stay separated under these moves: no two primitives at one distance along
    # any ray, so every tree gives the oracle's image of the moved mesh
    first = sp.Scene.from_file(sets[name][0])
    v, f = R.mesh_of(first)
    moved = R.MOVES[move](v, f)
    ref = {}
    for walk, options in WALKS.items():
        for builder in (("host", "device") if walk == "wide" else ("host",)):
            s = load(sets[name][0], builder=builder, **options)
            s.update_mesh(moved)
            assert np.array_equal(R.mesh_of(s)[0].view(np.uint32), moved.view(np.uint32))
            for i, spp in INTEGRATORS:
                if i not in ref:
                    ref[i] = oracle_of(s, i, spp)  # renders s.desc(): the moved mesh
                g, gst = sp.render_tiles(s, i, spp)
                assert (gst.stack_depth == 0) == (walk == "stackless")
                bit_exact(g, gst, *ref[i], (name, move, walk, builder, i))
                assert g.max() > 0.0


@pytest.mark.parametrize("move", ["shift", "bend"])
def test_bunny_within_the_sah_bar(scene_dir, move):
    path = os.path.join(scene_dir, "bunny.sp")
    fresh = load(path, upload=False)
    v, f = R.mesh_of(fresh)
    moved = R.shift(v, f) if move == "shift" else R.bend(v, f, 0.2)
    assert fresh.update_mesh(moved, stats=True)["refitted"] == 0
    fresh.upload(device=0)
    for i, spp in (("direct_lighting", 4), ("iterative_rrnee", 2)):
        c, cst = oracle_of(fresh, i, spp)
        # the input itself: a fresh SAH upload of the moved mesh is inside the bar
        g, gst = sp.render_tiles(fresh, i, spp)
        within_sah_bar(g, c)
        assert gst.rays == cst["rays"] and gst.shadow_rays == cst["shadow_rays"]
        for builder in R.BUILDERS:
            s = load(path, builder=builder)
            assert s.update_mesh(moved, stats=True)["refitted"] == 1
            assert s.bvh_check()["errors"] == 0 and s.wide_check()["errors"] == 0
            g, gst = sp.render_tiles(s, i, spp)
            print(move, i, builder, "rays", gst.rays, cst["rays"])
            within_sah_bar(g, c)
            assert gst.rays == cst["rays"] and gst.shadow_rays == cst["shadow_rays"]


def test_normals_follow_when_given(scene_dir):
    # flipped normals change the shading of a resident scene exactly as they change a fresh upload's
    path = os.path.join(scene_dir, "bunny.sp")
    s = load(path)
    d = s.desc()
    n0 = np.ctypeslib.as_array(d.normals, shape=(d.info.num_vertices, 3)).copy()
    v, f = R.mesh_of(s)
    kept, _ = sp.render_tiles(s, "direct_lighting", 2)
    s.update_mesh(v)  # normals not given: kept
    again, _ = sp.render_tiles(s, "direct_lighting", 2)
    assert np.array_equal(kept.view(np.uint32), again.view(np.uint32))
    s.update_mesh(v, normals=-n0)
    g, _ = sp.render_tiles(s, "direct_lighting", 2)
    fresh = load(path, upload=False)
    fresh.update_mesh(v, normals=-n0)
    fresh.upload(device=0)
    c, _ = sp.render_tiles(fresh, "direct_lighting", 2)
    assert np.array_equal(g.view(np.uint32), c.view(np.uint32))
    assert not np.array_equal(g.view(np.uint32), kept.view(np.uint32))


# ---------------------------------------------------------------- state
def test_reupload_after_a_refit_builds_from_the_new_mesh(sets):
    # nothing stale is left in the host mesh, and an upload after a refit builds again even with the
    # resident options (the resident topology is an earlier pose's)
    for builder in R.BUILDERS:
        s = load(sets["tri257"][0], builder=builder)
        v, f = R.mesh_of(s)
        moved = R.permute(v, f)
        fresh = R.moved_scene(s, moved)
        hb, hw = fresh.bvh_build_check(builder=builder), fresh.wide_build_check(builder=builder)
        s.update_mesh(moved)
        refitted = picked(s.bvh_check(), s.wide_check(), HASHES)
        assert refitted[0] != hb["hash"]  # A's topology with B's boxes is not B's tree
        s.upload(device=0, builder=builder)
        b, w = s.bvh_check(), s.wide_check()
        assert b["errors"] == 0 and w["errors"] == 0 and b["builder"] == builder
        assert picked(b, w, HASHES) == picked(hb, hw, HASHES), (builder, b, w, hb, hw)
        s.upload(device=0, builder=builder)  # resident again: no third build, the same arrays
        assert picked(s.bvh_check(), s.wide_check(), HASHES) == picked(hb, hw, HASHES)


def test_progress_objects(scene_dir):
    s = load(os.path.join(scene_dir, "bunny.sp"))
    v, f = R.mesh_of(s)
    old = sp.Progressive(s, "direct_lighting")
    old.render(1)
    s.update_mesh(R.shift(v, f))
    with pytest.raises(sp.SimplePathError) as e:
        old.render(1)
    assert e.value.code == _abi.SP_ERR_STATE
    old.close()
    one, _ = sp.render_tiles(s, "direct_lighting", 4)
    new = sp.Progressive(s, "direct_lighting")
    new.render(1)
    two, _ = new.render(3)
    new.close()
    assert np.array_equal(one.view(np.uint32), two.view(np.uint32))


def test_argument_rules_on_a_resident_scene(scene_dir):
    path = os.path.join(scene_dir, "bunny.sp")
    # the reference order is not refitted
    s = load(path, bvh_mode=1)
    v, f = R.mesh_of(s)
    before, _ = sp.render_tiles(s, "direct_lighting", 2)
    with pytest.raises(sp.SimplePathError) as e:
        s.update_mesh(R.shift(v, f))
    assert e.value.code == _abi.SP_ERR_ARG
    assert np.array_equal(R.mesh_of(s)[0].view(np.uint32), v.view(np.uint32))
    after, _ = sp.render_tiles(s, "direct_lighting", 2)
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
    # a refused update leaves a bvh_mode 0 residency and its progress objects as they were
    s = load(path)
    before, _ = sp.render_tiles(s, "direct_lighting", 2)
    prog = sp.Progressive(s, "direct_lighting")
    prog.render(1)
    with pytest.raises(sp.SimplePathError) as e:
        s.update_mesh(R.shift(v, f)[:-1])
    assert e.value.code == _abi.SP_ERR_ARG
    u = _abi.sp_mesh_update()
    u.struct_size = C.sizeof(_abi.sp_mesh_update)
    u.num_vertices = v.shape[0]
    assert sp.lib().sp_scene_update_mesh(s.handle, C.byref(u), None) == _abi.SP_ERR_ARG  # null vertices
    prog.render(1)
    prog.close()
    after, _ = sp.render_tiles(s, "direct_lighting", 2)
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
    assert s.bvh_check()["errors"] == 0
